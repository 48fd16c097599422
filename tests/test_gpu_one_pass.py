"""The one-kernel ray route (trace_kernel; RAIDER_HIP_ONE_PASS, default on) must not move a single bit.

An eligible raytrace() - one f32 lon/lat cube on exactly uniform axes, one slice of GRID rays with per-pixel look vectors in device arrays,
2 < K <= 128 - probes the slice's partition on the border tiles of the scene and a coarse lattice, fits and marches every ray in one
kernel on that partition, and then proves the partition from the maxima of every ray.  Where the proof fails - a longer ray in a tile the
probe did not visit, a NaN ray, a ray for the generic kernels - the two classic passes run behind it on the device and overwrite every
output.  Either way the caller must get what RAIDER_HIP_ONE_PASS=0 gives, bit for bit; Context.one_pass_count / one_pass_redo_count say
which way a call went.

The switch is read once per process: every scene below is traced by two fresh child processes, switch 0 and switch 1, once for the whole
module; the tests compare what the two wrote.  Cube: 24 x 24 x 12, f32, values as synthetic_cube, K = 11 levels under zref.  Scenes:
88 x 104 rays = 6 x 7 tiles, the last column and row of tiles padded, 4 x 5 interior tiles of which the probe's lattice visits one."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
NX, NY = 88, 104
PLACES = [(21, 21), (37, 53), (69, 69), (53, 37), (21, 85), (69, 21)]     # (column, row): six different interior tiles, (4, 4) the lattice's

CHILD = r'''
import sys
import numpy as np
import torch
sys.path.insert(0, %(root)r)
import raider_amd as R
from oracle import raider_oracle as O

out = {}
NX, NY = %(nx)d, %(ny)d
PLACES = %(places)r
dev = torch.device('cuda:0')
xp = np.linspace(-119.5, -115.5, NX); yp = np.linspace(34.5, 31.5, NY)
xx, yy = np.meshgrid(xp, yp)
ctx = R.Context.default()


def los_of(inc):
    return np.ascontiguousarray(O.look_vectors_from_inc_hd(inc, np.full(yy.shape, -167.9), yy, xx, 0.0))


def rays_of(los, **kw):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return R.Rays.grid(t(xp), t(yp), los=t(los), **{k: t(v) for k, v in kw.items()})


def host(a):
    return a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)


def run(tag, gpu, zref, los, ht=0.0, max_seg=1000.0, **kw):
    """the asynchronous call, then the synchronous one; counters after each"""
    c0, r0 = ctx.one_pass_count(), ctx.one_pass_redo_count()
    w, h, _, _ = gpu.raytrace(rays_of(los, **kw), ht, zref, max_seg=max_seg, want_nparts=False)
    out[tag + '.async.wet'] = host(w); out[tag + '.async.hyd'] = host(h)
    try:
        w, h, npt, fl = gpu.raytrace(rays_of(los, **kw), ht, zref, max_seg=max_seg, want_nparts=True)
        out[tag + '.wet'] = host(w); out[tag + '.hyd'] = host(h); out[tag + '.nparts'] = npt; out[tag + '.flags'] = np.int64(fl)
    except Exception as e:                                       # the library's verdict on the scene is part of the record
        out[tag + '.error'] = np.array(type(e).__name__ + ': ' + str(e))
    out[tag + '.nslow'] = np.int64(ctx.generic_ray_count())
    out[tag + '.calls'] = np.int64(ctx.one_pass_count() - c0)
    out[tag + '.redos'] = np.int64(ctx.one_pass_redo_count() - r0)


cube = O.synthetic_cube(24, 24, 12, seed=5)
gpu = R.Cube(cube['ys'], cube['xs'], cube['zs'], cube['wet'], cube['hydro'], order='zyx')
zref = float(cube['zs'].max() - 1)
inc = np.broadcast_to(np.linspace(30.0, 46.0, NX), yy.shape).copy()
smooth = los_of(inc)
run('smooth', gpu, zref, smooth)
for j, (col, row) in enumerate(PLACES):                          # one long ray, tile by tile: the probe cannot have seen most of them
    steep = inc.copy(); steep[row, col] = 62.0
    run('steep%%d' %% j, gpu, zref, los_of(steep), max_seg=200.0)
los = smooth.copy(); los[40, 37] = np.nan
run('nan', gpu, zref, los)
grazing = inc.copy(); grazing[40, 37] = 88.0                     # cos(inc) < 0.05: left to the generic kernels
run('generic', gpu, zref, los_of(grazing))
# calls the route does not take
run('few_levels', gpu, float(cube['zs'][2] - 1), smooth)         # K = 2
cube140 = O.synthetic_cube(24, 24, 140, seed=6)
gpu140 = R.Cube(cube140['ys'], cube140['xs'], cube140['zs'], cube140['wet'], cube140['hydro'], order='zyx')
out['levels140.K'] = np.int64(len(gpu140.ray_levels(0.0, float(cube140['zs'].max() - 1))[0]))
run('levels140', gpu140, float(cube140['zs'].max() - 1), smooth)
run('heights', gpu, zref, smooth, ht=None, hts=np.broadcast_to(np.linspace(0.0, 900.0, NX), yy.shape).copy())
gpu64 = R.Cube(cube['ys'], cube['xs'], cube['zs'], cube['wet_total'], cube['hydro_total'], order='zyx')
run('f64', gpu64, zref, smooth)
c0 = ctx.one_pass_count()
w, h, K, npt, fl = gpu.raytrace_slices(rays_of(smooth), np.array([0.0, 500.0]), zref)
out['slices.wet'] = host(w); out['slices.hyd'] = host(h); out['slices.nparts'] = npt; out['slices.calls'] = np.int64(ctx.one_pass_count() - c0)
np.savez(sys.argv[1], **out)
'''


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp('one_pass')
    got = []
    for switch in ('0', '1'):
        path = d / f'switch{switch}.npz'
        env = dict(os.environ, RAIDER_HIP_ONE_PASS=switch)
        res = subprocess.run([sys.executable, '-c', CHILD % dict(root=str(ROOT), nx=NX, ny=NY, places=PLACES), str(path)],
                             capture_output=True, text=True, timeout=300, env=env)
        assert res.returncode == 0, res.stderr[-3000:]
        got.append(dict(np.load(path)))
    return got


def _same(runs, tag, need):
    """every record of the scene but the route's own counters is bit for bit the same with the switch off and on"""
    off, on = runs
    keys = sorted(k for k in off if k.startswith(tag + '.'))
    assert keys == sorted(k for k in on if k.startswith(tag + '.')), (keys, sorted(on))
    assert off.get(tag + '.calls', 0) == 0 and off.get(tag + '.redos', 0) == 0
    for n in need:
        assert tag + '.' + n in keys, (n, keys)
    for k in keys:
        if k.endswith('.calls') or k.endswith('.redos'):
            continue
        a, b = off[k], on[k]
        if a.dtype.kind == 'f':
            assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(a.view(np.uint64), b.view(np.uint64)), k
        else:
            assert np.array_equal(a, b), (k, a, b)


def _scene():
    from oracle import raider_oracle as O
    xp = np.linspace(-119.5, -115.5, NX); yp = np.linspace(34.5, 31.5, NY)
    xx, yy = np.meshgrid(xp, yp)
    inc = np.broadcast_to(np.linspace(30.0, 46.0, NX), yy.shape).copy()
    los = np.ascontiguousarray(O.look_vectors_from_inc_hd(inc, np.full(yy.shape, -167.9), yy, xx, 0.0))
    cube = O.synthetic_cube(24, 24, 12, seed=5)
    return cube, xp, yp, los, float(cube['zs'].max() - 1)


def test_smooth_scene_takes_the_route_and_changes_nothing(runs):
    _same(runs, 'smooth', ('async.wet', 'async.hyd', 'wet', 'hyd', 'nparts', 'flags'))
    on = runs[1]
    assert on['smooth.calls'] == 2 and on['smooth.redos'] == 0          # (the asynchronous and the synchronous call)
    assert np.isfinite(on['smooth.wet']).all() and on['smooth.nslow'] == 0
    assert np.array_equal(on['smooth.async.wet'].view(np.uint64), on['smooth.wet'].view(np.uint64))


def test_smooth_scene_against_the_c_oracle(runs):
    """a block across a tile corner, an interior tile and the padded last column of tiles, with the whole slice's partition: 1e-9 m"""
    from oracle import oracle_c as OC
    cube, xp, yp, los, zref = _scene()
    _, _, onp = OC.build_cube_ray_slice(cube, xp, yp, 0.0, los, zref)
    rows, cols = slice(28, 52), slice(60, 88)
    ow, oh, _ = OC.build_cube_ray_slice(cube, xp[cols], yp[rows], 0.0, np.ascontiguousarray(los[rows, cols]), zref, nparts=onp)
    for r in runs:
        assert np.array_equal(r['smooth.nparts'], onp)
        err = max(np.abs(r['smooth.wet'][rows, cols] - ow).max(), np.abs(r['smooth.hyd'][rows, cols] - oh).max())
        print('smooth scene, block against oracle_c:', err, 'm')
        assert err <= 1e-9


def test_a_partition_the_probe_missed_is_redone(runs):
    on = runs[1]
    redone = 0
    for j in range(len(PLACES)):
        tag = 'steep%d' % j
        _same(runs, tag, ('async.wet', 'wet', 'hyd', 'nparts', 'flags'))
        assert on[tag + '.calls'] == 2
        assert (on[tag + '.nparts'] >= runs[1]['smooth.nparts']).all() and on[tag + '.nparts'].max() > 10      # max_seg = 200 and a 62 degree ray
        redone += int(on[tag + '.redos'] >= 1)
    print('placements whose classic passes ran:', redone, 'of', len(PLACES))
    assert redone >= 1


def test_a_nan_look_vector(runs):
    _same(runs, 'nan', ('async.wet', 'async.hyd', 'error'))
    on = runs[1]
    assert np.isnan(on['nan.async.wet']).all() and np.isnan(on['nan.async.hyd']).all()      # the partition is undefined: every output of the slice
    assert 'NaN' in str(on['nan.error']) and on['nan.calls'] == 2


def test_one_generic_ray(runs):
    _same(runs, 'generic', ('async.wet', 'wet', 'hyd', 'nparts', 'flags', 'nslow'))
    on = runs[1]
    assert on['generic.nslow'] == 1 and on['generic.calls'] == 2 and on['generic.redos'] >= 1
    # (the grazing ray itself runs out of the cube's side: NaN, as the reference's interpolator fills it; every other ray is finite)
    assert np.isfinite(np.delete(on['generic.wet'].ravel(), 40 * NX + 37)).all()


@pytest.mark.parametrize('tag', ['few_levels', 'levels140', 'heights', 'f64'])
def test_calls_that_are_not_eligible(runs, tag):
    _same(runs, tag, ('async.wet', 'wet', 'hyd', 'nparts', 'flags'))
    on = runs[1]
    assert on[tag + '.calls'] == 0 and on[tag + '.redos'] == 0
    if tag == 'few_levels':
        assert on['few_levels.nparts'].size == 2
    if tag == 'levels140':
        assert on['levels140.K'] > 128


def test_two_slices_are_not_eligible(runs):
    _same(runs, 'slices', ('wet', 'hyd', 'nparts'))
    assert runs[1]['slices.calls'] == 0
    assert np.array_equal(runs[1]['slices.wet'][0].view(np.uint64), runs[1]['smooth.wet'].view(np.uint64))


def test_want_nparts_returns_the_exact_partition(runs):
    """on the route the maxima every ray folded - not the probed ones - are what comes back: the two-pass partition, and the oracle's"""
    from oracle import oracle_c as OC
    cube, xp, yp, los, zref = _scene()
    off, on = runs
    for tag in ['smooth'] + ['steep%d' % j for j in range(len(PLACES))]:
        assert np.array_equal(on[tag + '.nparts'], off[tag + '.nparts']) and on[tag + '.flags'] == off[tag + '.flags']
    xx, yy = np.meshgrid(xp, yp)
    from oracle import raider_oracle as O
    inc = np.broadcast_to(np.linspace(30.0, 46.0, NX), yy.shape).copy()
    col, row = PLACES[0]
    inc[row, col] = 62.0
    steep = np.ascontiguousarray(O.look_vectors_from_inc_hd(inc, np.full(yy.shape, -167.9), yy, xx, 0.0))
    _, _, onp = OC.build_cube_ray_slice(cube, xp, yp, 0.0, steep, zref, max_seg=200.0)
    assert np.array_equal(on['steep0.nparts'], onp)
