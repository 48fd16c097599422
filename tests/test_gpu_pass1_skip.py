"""Pass 1's wave-level skip of the per-level length loop (RAIDER_HIP_PASS1_SKIP, default on) must not move a single bit.

The switch is read once per process, so every scene below is traced by two child processes - switch 0 and switch 1 - once for the
whole module; the tests compare what the two wrote.  A scene's record holds the prepass maxima and flags, the delays, nParts and
flags of raytrace(), the number of rays left to the generic kernels, or the text of the exception where the library raises one.
Results never show whether a wave skipped, so the prepass also reports how many did (Context.skipped_wave_count): 0 with the switch off,
and well above 0 with it on wherever the scene lets a workgroup see long rays before shorter ones.

A workgroup can only skip from its second tile on (its floor starts at 0), so the scenes must have many more tiles than the launch has
workgroups: 1024 x 500 rays are 64 x 32 = 2048 tiles (the last row of tiles padded: 500 = 31 x 16 + 4), and the children run with
RAIDER_HIP_BLOCKS_PER_CU=1, one workgroup per CU - about 8 tiles each, taken from a band of 4 tile rows in whatever order the walk
hands them out.  The cube is the 12 x 12 x 10 synthetic one; incidence goes from 20 to 50 deg across the columns unless stated otherwise."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, %(root)r)
import raider_amd as R
from oracle import raider_oracle as O

out = {}
NX, NY = 1024, 500
xp = np.linspace(-119.5, -115.5, NX); yp = np.linspace(34.5, 31.5, NY)
xx, yy = np.meshgrid(xp, yp)


def los_of(inc, xx=xx):
    return np.ascontiguousarray(O.look_vectors_from_inc_hd(inc, np.full(yy.shape, -167.9), yy, xx, 0.0))


def run(tag, gpu, zref, xpts, los, ht=0.0):
    ctx = R.Context.default()
    for name, call in (('pre', lambda: gpu.ray_prepass(R.Rays.grid(xpts, yp, los=los), ht, zref)),
                       ('ray', lambda: gpu.raytrace(R.Rays.grid(xpts, yp, los=los), ht, zref, want_nparts=True))):
        try:
            res = call()
            if name == 'pre':
                out[tag + '.maxlen'] = res[0]; out[tag + '.preflags'] = np.int64(res[1])
                out[tag + '.nslow'] = np.int64(ctx.generic_ray_count()); out[tag + '.nskip'] = np.int64(ctx.skipped_wave_count())
            else:
                out[tag + '.wet'] = res[0]; out[tag + '.hyd'] = res[1]; out[tag + '.nparts'] = res[2]; out[tag + '.flags'] = np.int64(res[3])
        except Exception as e:                                   # the library's verdict on the scene is part of the record
            out[tag + '.' + name + '.error'] = np.array(type(e).__name__ + ': ' + str(e))


cube = O.synthetic_cube(12, 12, 10, seed=3)
gpu = R.Cube(cube['ys'], cube['xs'], cube['zs'], cube['wet'], cube['hydro'], order='zyx')
zref = float(cube['zs'].max() - 1)
inc = np.broadcast_to(np.linspace(20.0, 50.0, NX), yy.shape).copy()
base = los_of(inc)
run('base', gpu, zref, xp, base)
# the same rays with the columns in the opposite order: the steepest tiles come last instead of first
run('reversed', gpu, zref, xp[::-1].copy(), np.ascontiguousarray(base[:, ::-1]))
# one incidence everywhere: every wave ties with the floor the first tiles set
run('constant', gpu, zref, xp, los_of(np.full(yy.shape, 37.0)))
# waves that must not skip; each scene also has a ray in the LAST tile, longer than everything before it
inc_late = inc.copy(); inc_late[NY - 1, NX - 1] = 62.0
los = los_of(inc_late); los[2, 3] = np.nan
run('nan', gpu, zref, xp, los)
inc_g = inc_late.copy(); inc_g[5, 200] = 88.0                    # cos(inc) < 0.05: left to the generic kernel
run('generic', gpu, zref, xp, los_of(inc_g))
los = los_of(inc_late); los[1, 1] *= 1e-3; los[200, 300] *= 3.0   # look vectors that are not unit vectors
run('nonunit', gpu, zref, xp, los)
# three slices in one launch: floor and table belong to a slice
try:
    w, h, K, npt, fl = gpu.raytrace_slices(R.Rays.grid(xp, yp, los=base), np.array([0.0, 500.0, 3000.0]), zref)
    out['slices.wet'] = w; out['slices.hyd'] = h; out['slices.K'] = K; out['slices.nparts'] = npt; out['slices.flags'] = fl
except Exception as e:
    out['slices.error'] = np.array(type(e).__name__ + ': ' + str(e))
# 70 levels (74 nodes: the three intervals that end below the rays' height 0 are no levels): lanes bound two levels each
cube70 = O.synthetic_cube(12, 12, 74, seed=4)
gpu70 = R.Cube(cube70['ys'], cube70['xs'], cube70['zs'], cube70['wet'], cube70['hydro'], order='zyx')
zref70 = float(cube70['zs'].max() - 1)
out['levels70.K'] = np.int64(len(gpu70.ray_levels(0.0, zref70)[0]))
run('levels70', gpu70, zref70, xp, base)
np.savez(sys.argv[1], **out)
'''


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp('pass1_skip')
    got = []
    for switch in ('0', '1'):
        path = d / f'switch{switch}.npz'
        env = dict(os.environ, RAIDER_HIP_PASS1_SKIP=switch, RAIDER_HIP_BLOCKS_PER_CU='1')
        res = subprocess.run([sys.executable, '-c', CHILD % dict(root=str(ROOT)), str(path)], capture_output=True, text=True, timeout=300, env=env)
        assert res.returncode == 0, res.stderr[-3000:]
        got.append(dict(np.load(path)))
    return got


def _same(runs, tag, need):
    off, on = runs
    keys = sorted(k for k in off if k.startswith(tag + '.'))
    assert keys == sorted(k for k in on if k.startswith(tag + '.')), (keys, sorted(on))
    if tag + '.nskip' in keys:
        assert off[tag + '.nskip'] == 0, off[tag + '.nskip']
        keys.remove(tag + '.nskip')
    for n in need:
        assert tag + '.' + n in keys, (n, keys)
    for k in keys:
        a, b = off[k], on[k]
        if a.dtype.kind == 'f':
            assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), k     # bit for bit, NaNs included
        else:
            assert np.array_equal(a, b), (k, a, b)


def test_switch_changes_nothing(runs):
    _same(runs, 'base', ('maxlen', 'preflags', 'nslow', 'wet', 'hyd', 'nparts', 'flags'))
    assert runs[1]['base.nslow'] == 0 and (runs[1]['base.maxlen'] > 0).all() and np.isfinite(runs[1]['base.wet']).all()
    # Skipping really happens.  A tile skips when its workgroup has already had a tile far enough to the right; of a workgroup's ~8 tiles,
    # drawn in any order, the j-th is to the right of all earlier ones with probability 1/j, so about 1 - H(8)/8 = 66 % of the waves can
    # skip, less the columns within the bound's slack of the floor.  A quarter of the 8192 waves is a safe floor for "it happens".
    print('skipped waves, base scene:', int(runs[1]['base.nskip']), 'of', 2048 * 4)
    assert runs[1]['base.nskip'] > 2048


def test_order_of_the_tiles_does_not_matter(runs):
    _same(runs, 'reversed', ('maxlen', 'nparts'))
    _same(runs, 'constant', ('maxlen', 'nparts', 'wet'))
    assert runs[1]['reversed.nskip'] > 2048
    for r in runs:
        assert np.array_equal(r['reversed.maxlen'].view(np.uint64), r['base.maxlen'].view(np.uint64))
        assert np.array_equal(r['reversed.wet'][:, ::-1].view(np.uint64), np.ascontiguousarray(r['base.wet']).view(np.uint64))


@pytest.mark.parametrize('tag', ['nan', 'generic', 'nonunit'])
def test_waves_that_must_not_skip(runs, tag):
    _same(runs, tag, ('maxlen', 'preflags', 'nslow'))
    on = runs[1]
    if tag == 'generic':
        assert on['generic.nslow'] == 1
    assert on[tag + '.nskip'] > 0                              # the other waves of the scene still skip
    # the late, longest ray of the scene still raised the maxima (from level 1 on: beyond the base scene's)
    assert (on[tag + '.maxlen'][1:] > on['base.maxlen'][1:]).all()
    if tag == 'nan':
        assert int(on['nan.preflags']) & 1                     # FLAG_ANY_NAN: the NaN poisoning of the slice maximum


def test_slices_in_one_launch(runs):
    _same(runs, 'slices', ('wet', 'hyd', 'K', 'nparts', 'flags'))
    on = runs[1]
    assert np.array_equal(on['slices.wet'][0].view(np.uint64), on['base.wet'].view(np.uint64))
    assert np.array_equal(on['slices.nparts'][0][:on['slices.K'][0]], on['base.nparts'])


def test_more_than_64_levels(runs):
    assert runs[1]['levels70.K'] == 70 and runs[1]['levels70.nskip'] > 2048
    _same(runs, 'levels70', ('maxlen', 'preflags', 'wet', 'hyd', 'nparts', 'flags'))


def test_nparts_against_the_c_oracle(runs):
    from oracle import oracle_c as OC
    from oracle import raider_oracle as O
    xp = np.linspace(-119.5, -115.5, 1024); yp = np.linspace(34.5, 31.5, 500)
    xx, yy = np.meshgrid(xp, yp)
    inc = np.broadcast_to(np.linspace(20.0, 50.0, 1024), yy.shape).copy()
    los = np.ascontiguousarray(O.look_vectors_from_inc_hd(inc, np.full(yy.shape, -167.9), yy, xx, 0.0))
    cube = O.synthetic_cube(12, 12, 10, seed=3)
    _, _, onp = OC.build_cube_ray_slice(cube, xp, yp, 0.0, los, float(cube['zs'].max() - 1))
    for r in runs:
        assert np.array_equal(r['base.nparts'], onp)
