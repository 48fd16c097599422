"""Every instantiation of the two ray passes against the oracle (DESIGN.md "the ray passes' pins").

The host picks one kernel instantiation per call (raider_hip.hip: crossings_fn, march_fn, march_epochs_fn, march_grid, epoch_group, and
the two generic kernels).  The other comparisons with the oracle reach a handful of them by accident of scene; the rest hang on
route-against-route tests.  Here a covering table of small cases reaches EVERY one, and the selectors are restated in Python (`_reached`):
each case first asserts from that model which instantiation it runs - applied on the GPU to the very Cube and Rays objects handed to the
library - and only then looks at a delay.  A case that lands elsewhere fails with the name of the instantiation it does reach.

  pass 1, light     2 dtypes x {lon/lat, conic} x OM {0, 1, 2} x per-ray heights {no, yes}           24   (+ one polar-stereographic case)
  pass 1, generic   2 dtypes                                                                          2
  pass 2, light     per dtype REGULAR / TABLES / flags, per-ray heights on REGULAR and flags          10
  pass 2, generic   2 dtypes                                                                          2
  pass 2, stacked   the same 10 x E in {2, 4}                                                         20

Scene: 21 x 37 rays (partial 16 x 16 tiles both ways) on a 40 x 44 x 24 cube, hanging over one cube edge (50 % .. 95 % of the
reference's outputs finite: a CPU test); incidence 20 .. 50 degrees across the scene; slices at 0 m and 300 m, or per-ray heights: a
ramp 0 .. 1500 m with the planted values of test_gpu_perpixel.py::test_mixed_heights_against_the_oracle (on a model node, 0.4 m below
one, 0.3 m above one, and half a metre above the cube's lowest node, which becomes the height of the level table).

Reference: oracle_c.build_cube_ray_slice / build_cube_ray_per_pixel (the latter with the model projection added for this module and
pinned below on the CPU), raider_oracle.build_cube_ray for the polar-stereographic cube.  Checked per case: nParts, the NaN mask, and
|gpu - oracle| <= 5e-9 m = 5 * TIGHT on wet and hydro, the bound tests/test_gpu_parity.py uses for sweeps up to 60 degrees of incidence.
Every GPU test prints `RAYINST <case> <instantiations> <largest distance>`."""
import os
import re
from collections import namedtuple
from pathlib import Path

import numpy as np
import pytest

from oracle import raider_oracle as O
from oracle import oracle_c as OC

TIGHT = 1e-9
TOL = 5 * TIGHT                 # metres
NY, NX = 21, 37
CUBE = (40, 44, 24)
SLICES = (0.0, 300.0)
HD = -167.9

# ---- the model of the selectors ------------------------------------------------------------------------------------------------------


def _thresholds():
    """(exact, uni) of axis_uniformity, read out of raider_hip.hip"""
    src = (Path(__file__).resolve().parent.parent / 'raider_amd' / 'csrc' / 'raider_hip.hip').read_text()
    num = r'([0-9]+\.?[0-9]*(?:[eE][-+]?[0-9]+)?)'
    uni = re.search(r'\*uni\s*=\s*worst\s*<\s*' + num + r'\s*\?\s*1\s*:\s*0', src)
    exact = re.search(r'\*exact\s*=\s*worst\s*<\s*' + num + r'\s*\?\s*1\s*:\s*0', src)
    assert uni and exact, 'axis_uniformity no longer compares `worst` with two plain constants: restate the model of march_grid'
    return float(exact.group(1)), float(uni.group(1))


def _axis_uniformity(g):
    """(uni, exact) as raider_hip.hip: axis_uniformity computes them"""
    t_exact, t_uni = _thresholds()
    g = np.asarray(g, dtype=np.float64)
    inv_d = (g.size - 1) / (g[-1] - g[0])
    worst = 0.0
    for i in range(g.size):
        worst = max(worst, abs((g[i] - g[0]) * inv_d - i))
    return bool(worst < t_uni), bool(worst < t_exact)


def _march_grid(ys, xs, per_ray):
    """raider_hip.hip: march_grid for a `small` cube"""
    (uy, ey), (ux, ex) = _axis_uniformity(ys), _axis_uniformity(xs)
    if ey and ex:
        return 'regular'
    return 'tables' if (not per_ray and not ey and not ex and uy and ux) else 'flags'


def _epoch_groups(D, f64, per_ray, env):
    """raider_hip.hip: launch_march_epochs' groups = engine.epoch_groups under epochs_max and epoch_group's cap"""
    from raider_amd.engine import epoch_groups
    emax = int(env.get('RAIDER_HIP_EPOCHS_MAX', 4))
    if per_ray and f64:
        emax = min(emax, int(env.get('RAIDER_HIP_EPOCHS_PR_F64_MAX', 2)))
    return epoch_groups(D, emax)


def _generic_rays(proj, xs, lat, lon, los, hts, zref):
    """How many rays the static classification of pass 1 (raider_kernels.h: fast_ok) sends to the generic kernels.  The scenes keep
    every ray far from its thresholds, so round-off cannot move the count."""
    la, lo = np.radians(np.ravel(lat)), np.radians(np.ravel(lon))
    los = np.reshape(los, (-1, 3))
    up = np.stack([np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)], -1)
    cosi = (los * up).sum(-1) / np.linalg.norm(los, axis=-1)
    gam = (zref - np.broadcast_to(hts, np.shape(lat)).ravel()) / (cosi * 6.3e6)
    c0 = np.cos(la)
    lon = np.ravel(lon)
    if proj is not None:
        dl = lon - proj['lon_0']
        dl = dl - 360.0 * np.rint(dl / 360.0)
        ok = (np.abs(dl) + 12.0 < 180.0) & (proj.get('es', 0.0) == 0.0) & (gam < 0.09 * c0)
    else:
        wrap_pos = xs.max() <= 180.0 and xs.min() > -168.0
        wrap_neg = xs.min() >= -180.0 and xs.max() < 168.0
        ok = (np.abs(lon) + 5.0 < 180.0) | ((np.abs(lon) <= 180.0) & np.where(lon > 0.0, wrap_pos, wrap_neg))
    fast = (cosi > 0.05) & (c0 > gam + 0.02) & (gam < 0.12 * (c0 - gam)) & (gam < 0.035) & ok
    return int((~fast).sum())


def _reached(f64, proj, ys, xs, grid_origin, los_vec, per_ray, D, n_generic, n_active, env):
    """The set of instantiations one call launches ON RAYS: names as in the table of the module docstring"""
    t = 'f64' if f64 else 'f32'
    hk = 'pr' if per_ray else 'slice'
    if n_generic == n_active:
        return {f'crossings<{t},generic>', f'march<{t},generic>'}
    if n_generic != 0:
        return {f'mixed<{n_generic} of {n_active} rays generic>'}
    om = 0 if not grid_origin else (1 if los_vec else 2)
    out = {f'crossings<{t},{"conic" if proj is not None else "lonlat"},om{om},{hk}>'}
    grid = _march_grid(ys, xs, per_ray)
    for g in _epoch_groups(D, f64, per_ray, env):
        out.add(f'march<{t},{grid},{hk}>' if g == 1 else f'march_epochs<{t},E{g},{grid},{hk}>')
    return out


# ---- the case table ------------------------------------------------------------------------------------------------------------------
# crs: lonlat | lcc (HRRR's spherical cone) | stere (HRRR-AK) | polar (lon/lat at the pole: generic) | elcc (ellipsoidal cone: generic)
# axes: regular | tables | flags (tests/test_gpu_epochs.py::_fold_axes); form: grid_los | grid_inc | llh_los | xyz_los
Case = namedtuple('Case', 'id f64 crs axes form per_ray D env want')

# HRRR's cone (test_series_equals_per_date_lcc_and_polar_stereographic) with a false origin: on x_0 = y_0 = 0 a kernel that lost
# proj.x0 or proj.y0 would pass
LCC = dict(lat_1=38.5, lat_2=38.5, lat_0=38.5, lon_0=262.5, x_0=2.5e6, y_0=1.0e6, a=6371229.0, es=0.0)
STERE = dict(proj='stere', lat_0=90.0, lat_ts=60.0, lon_0=225.0, a=6371229.0, es=0.0)
ELCC = dict(lat_1=33.0, lat_2=45.0, lat_0=38.5, lon_0=-97.5, x_0=1000.0, y_0=-2000.0, a=6378137.0, es=0.0066943799901413165)
PROJ = dict(lonlat=None, polar=None, lcc=LCC, stere=STERE, elcc=ELCC)
AXES = ('regular', 'tables', 'flags')
GRID_OF = {('regular', False): 'regular', ('regular', True): 'regular', ('tables', False): 'tables', ('tables', True): 'flags',
           ('flags', False): 'flags', ('flags', True): 'flags'}


def _t(f64):
    return 'f64' if f64 else 'f32'


def _hk(per_ray):
    return 'pr' if per_ray else 'slice'


def _cases():
    out = []
    # pass 1, light: one case per instantiation; the axes kind rotates so that both CRS families reach every pass-2 instantiation
    for f64 in (False, True):
        for ci, crs in enumerate(('lonlat', 'lcc')):
            for per_ray in (False, True):
                for om in (0, 1, 2):
                    axes = AXES[(om + ci + f64) % 3]
                    form = ('llh_los' if (f64 + ci + per_ray) % 2 == 0 else 'xyz_los') if om == 0 else ('grid_los' if om == 1 else 'grid_inc')
                    grid = GRID_OF[axes, per_ray]
                    want = {f'crossings<{_t(f64)},{"conic" if ci else "lonlat"},om{om},{_hk(per_ray)}>', f'march<{_t(f64)},{grid},{_hk(per_ray)}>'}
                    out.append(Case(f'p1-{_t(f64)}-{crs}-om{om}-{_hk(per_ray)}-{grid}', f64, crs, axes, form, per_ray, 1, {}, want))
    out.append(Case('p1-f32-stere-om2-slice-regular', False, 'stere', 'regular', 'grid_inc', False, 1, {},
                    {'crossings<f32,conic,om2,slice>', 'march<f32,regular,slice>'}))
    # pass 2, stacked: one case per instantiation and E
    i = 0
    for f64 in (False, True):
        for grid, per_ray in (('regular', False), ('tables', False), ('flags', False), ('regular', True), ('flags', True)):
            for E in (2, 4):
                crs = ('lonlat', 'lcc')[(i + (E == 4)) % 2]
                axes = grid if not (per_ray and grid == 'flags' and E == 4) else 'tables'       # (per-ray heights on TABLES axes: flags too)
                form = ('grid_los', 'grid_inc', 'llh_los', 'xyz_los')[(i + E) % 4] if per_ray else ('grid_inc', 'grid_los', 'llh_los')[(i + E) % 3]
                env = {'RAIDER_HIP_EPOCHS_PR_F64_MAX': '4'} if (f64 and per_ray and E == 4) else {}
                om = 0 if form in ('llh_los', 'xyz_los') else (1 if form == 'grid_los' else 2)
                want = {f'crossings<{_t(f64)},{"conic" if crs == "lcc" else "lonlat"},om{om},{_hk(per_ray)}>',
                        f'march_epochs<{_t(f64)},E{E},{grid},{_hk(per_ray)}>'}
                out.append(Case(f'st-{_t(f64)}-E{E}-{grid}-{_hk(per_ray)}', f64, crs, axes, form, per_ray, E, env, want))
            i += 1
    # the generic kernels: every ray of the scene fails the static classification
    for f64 in (False, True):
        for crs in ('polar', 'elcc'):
            for per_ray in (False, True):
                out.append(Case(f'gen-{_t(f64)}-{crs}-{_hk(per_ray)}', f64, crs, 'regular', 'grid_inc' if crs == 'polar' else 'grid_los', per_ray, 1, {},
                                {f'crossings<{_t(f64)},generic>', f'march<{_t(f64)},generic>'}))
    return out


CASES = _cases()
SINGLE = [c for c in CASES if c.D == 1]
STACKED = [c for c in CASES if c.D > 1]

# ---- scenes and references (built once per case, never modified) ----------------------------------------------------------------------


def _base_cube(crs, seed):
    ny, nx, nz = CUBE
    if crs == 'lonlat':
        return O.synthetic_cube(ny, nx, nz, seed=seed)
    if crs == 'lcc':                   # the cube of the HRRR series test, moved by the false origin
        return O.synthetic_cube(ny, nx, nz, seed=seed, y0=-9.0e5 + LCC['y_0'], y1=1.0e5 + LCC['y_0'], x0=-2.2e6 + LCC['x_0'], x1=-1.3e6 + LCC['x_0'])
    if crs == 'polar':
        return O.synthetic_cube(ny, nx, nz, seed=seed, ztop=15000.0, y0=86.0, y1=89.9, x0=-60.0, x1=60.0)
    if crs == 'stere':
        c = O.synthetic_cube(ny, nx, nz, seed=seed)
        cx, cy = O.stere_forward(61.0, -150.0, **{k: v for k, v in STERE.items() if k != 'proj'})
        c['xs'] = cx + 6000.0 * (np.arange(nx) - nx // 2); c['ys'] = cy + 6000.0 * (np.arange(ny) - ny // 2)
        return c
    if crs == 'elcc':
        c = O.synthetic_cube(ny, nx, nz, seed=seed)
        cx, cy = O.lcc_forward(38.0, -105.7, **ELCC)
        c['xs'] = cx + 9000.0 * (np.arange(nx) - nx // 2); c['ys'] = cy + 9000.0 * (np.arange(ny) - ny // 2)
        return c
    raise KeyError(crs)


# the scene's lon / lat axes per CRS: over the cube's middle (where the stacked cases' NaN block lies) and across its eastern edge
SCENE_AXES = {
    'lonlat': ((-118.3, -112.4), (34.5, 31.5)),
    'lcc': ((-117.8, -110.6), (35.4, 32.0)),
    'stere': ((-151.3, -147.3), (61.5, 60.5)),
    'polar': ((-25.0, 66.0), (89.5, 88.95)),
    'elcc': ((-106.6, -103.4), (38.7, 37.3)),
}
HOLE = (slice(None), slice(16, 21), slice(17, 23))           # [z, y, x] of the NaN block of one epoch


def _fold_axes(c, kind):
    ys, xs = c['ys'].copy(), c['xs'].copy()
    if kind == 'tables':
        ys, xs = ys.astype(np.float32).astype(np.float64), xs.astype(np.float32).astype(np.float64)
    elif kind == 'flags':
        ys[5] += 0.25 * (ys[1] - ys[0])
    return ys, xs


def _heights(zs, lo=0.0, hi=1500.0, node=3, lowest=None):
    """a ramp lo .. hi over the scene and four planted values: on a model node, 0.4 m below the next one, 0.3 m above it, and the
    batch's lowest ray (default: half a metre above the cube's bottom node)"""
    h = lo + (hi - lo) * (0.5 * np.arange(NY)[:, None] / (NY - 1) + 0.5 * np.arange(NX)[None, :] / (NX - 1))
    assert lo < zs[node] < zs[node + 1] < hi
    h[3, 5] = zs[node]; h[4, 6] = zs[node + 1] - 0.4; h[5, 7] = zs[node + 1] + 0.3; h[2, 3] = zs[0] + 0.5 if lowest is None else lowest
    return h


_SCENES = {}


def _scene(case):
    """Everything a case hands to the library and to the oracle.  Epoch e: seed 10 + e, fields scaled by 1 + 0.03 e, and in epoch 1 of a
    series a NaN block over the scene (tests/test_gpu_epochs.py: _epochs / _wm)."""
    if case.id in _SCENES:
        return _SCENES[case.id]
    dt = np.float64 if case.f64 else np.float32
    cubes = []
    for e in range(case.D):
        c = _base_cube(case.crs, 10 + e)
        ys, xs = _fold_axes(c, case.axes)
        w, h = (c['wet'] * (1.0 + 0.03 * e)).astype(np.float32).astype(dt), (c['hydro'] * (1.0 + 0.03 * e)).astype(np.float32).astype(dt)
        if case.D > 1 and e == 1:
            w[HOLE] = np.nan; h[HOLE] = np.nan
        cubes.append(dict(ys=ys, xs=xs, zs=c['zs'], wet=w, hydro=h))
    zs = cubes[0]['zs']
    (xa, xb), (ya, yb) = SCENE_AXES[case.crs]
    xp, yp = np.linspace(xa, xb, NX), np.linspace(ya, yb, NY)
    xx, yy = np.meshgrid(xp, yp)
    inc = np.broadcast_to(20.0 + 30.0 * np.arange(NX) / (NX - 1), (NY, NX)).copy()
    hd = np.full((NY, NX), HD) if case.form.endswith('_inc') else np.random.default_rng(7).uniform(-180.0, 180.0, (NY, NX))
    if case.crs == 'polar':             # the geometry of test_series_with_generic_rays: heights inside the 15 km cube
        heights, hts = (9300.0, 9800.0), _heights(zs, 8800.0, 10800.0, node=18, lowest=8700.0)
    else:
        heights, hts = SLICES, _heights(zs)
    los = np.ascontiguousarray(O.look_vectors_from_inc_hd(inc, hd, yy, xx, 0.0))             # (independent of the height: enu2ecef)
    s = dict(cubes=cubes, proj=PROJ[case.crs], xp=xp, yp=yp, xx=xx, yy=yy, inc=inc, hd=hd, los=los, zref=float(zs.max() - 1),
             heights=None if case.per_ray else heights, hts=hts if case.per_ray else None)
    _SCENES[case.id] = s
    return s


def _model_reached(case):
    """the model applied to the scene's arrays (no device)"""
    s = _scene(case)
    c = s['cubes'][0]
    n = 0
    for h in ([s['hts']] if case.per_ray else s['heights']):
        n += _generic_rays(s['proj'], c['xs'], s['yy'], s['xx'], s['los'], h, s['zref'])
    active = NY * NX * (1 if case.per_ray else len(s['heights']))
    return _reached(c['wet'].dtype == np.float64, s['proj'], c['ys'], c['xs'], case.form.startswith('grid'), case.form.endswith('_los'),
                    s['hts'] is not None, case.D, n, active, case.env), n


_REFS = {}


def _reference(case):
    """[epoch] -> list over the slices (one entry for per-ray heights) of (wet, hydro, nparts) from the oracle"""
    if case.id in _REFS:
        return _REFS[case.id]
    s = _scene(case)
    out = []
    for c in s['cubes']:
        if case.per_ray:
            ref = [OC.build_cube_ray_per_pixel(c, s['yy'], s['xx'], s['hts'], s['los'], s['zref'], model_proj=s['proj'])]
        elif case.crs == 'stere':        # the C oracle has no stereographic projection
            ip = list(O.getInterpolators(c['xs'], c['ys'], c['zs'], c['wet'], c['hydro']))
            (w, h), nps = O.build_cube_ray(s['xp'], s['yp'], np.array(s['heights']), lambda ht, llh, xyz, yy: s['los'], ip,
                                           MAX_TROPO_HEIGHT=s['zref'], return_nparts=True, model_proj=s['proj'])
            ref = [(w[k], h[k], nps[k]) for k in range(len(s['heights']))]
        else:
            ref = [OC.build_cube_ray_slice(c, s['xp'], s['yp'], ht, s['los'], s['zref'], model_proj=s['proj']) for ht in s['heights']]
        out.append(ref)
    _REFS[case.id] = out
    return out


# ---- CPU: the census, the fixtures' condition, the oracle addition -------------------------------------------------------------------


def test_census_every_instantiation_is_reached_by_the_case_named_for_it():
    reached = {}
    for case in CASES:
        got, n_generic = _model_reached(case)
        assert got == case.want, f'{case.id} is named for {sorted(case.want)} and reaches {sorted(got)}'
        assert n_generic == (0 if not case.id.startswith('gen-') else NY * NX * (1 if case.per_ray else 2)), (case.id, n_generic)
        for name in got:
            reached.setdefault(name, []).append(case.id)
    assert len({c.id for c in CASES}) == len(CASES)
    T, H = ('f32', 'f64'), ('slice', 'pr')
    p1 = {f'crossings<{t},{k},om{om},{h}>' for t in T for k in ('lonlat', 'conic') for om in (0, 1, 2) for h in H}
    p2 = {f'march<{t},{g},{h}>' for t in T for g, h in (('regular', 'slice'), ('tables', 'slice'), ('flags', 'slice'), ('regular', 'pr'), ('flags', 'pr'))}
    st = {f'march_epochs<{t},E{E},{g},{h}>' for t in T for E in (2, 4)
          for g, h in (('regular', 'slice'), ('tables', 'slice'), ('flags', 'slice'), ('regular', 'pr'), ('flags', 'pr'))}
    gen = {f'{k}<{t},generic>' for k in ('crossings', 'march') for t in T}
    assert (len(p1), len(p2), len(st), len(gen)) == (24, 10, 20, 4)
    assert set(reached) == p1 | p2 | st | gen, (sorted((p1 | p2 | st | gen) - set(reached)), sorted(set(reached) - (p1 | p2 | st | gen)))
    # every light pass-2 instantiation from a lon/lat AND from a conic cube (single-cube cases)
    for name in p2:
        kinds = {c.crs for c in SINGLE if name in c.want}
        assert 'lonlat' in kinds and 'lcc' in kinds, (name, kinds)
    # the one polar-stereographic cube (the n = 1 cone) and both families of generic scene
    assert sum(c.crs == 'stere' for c in CASES) == 1 and {c.crs for c in CASES if c.id.startswith('gen-')} == {'polar', 'elcc'}
    # half of the OM 0 cases of the pass-1 table start from lat / lon, half from ECEF
    om0 = [c.form for c in SINGLE if c.id.startswith('p1-') and '-om0-' in c.id]
    assert len(om0) == 8 and om0.count('llh_los') == 4 and om0.count('xyz_los') == 4


def test_the_model_reads_the_axes_as_the_host_does():
    t_exact, t_uni = _thresholds()
    assert 0.0 < t_exact < 1e-6 < t_uni < 0.5
    c = _base_cube('lonlat', 10)
    kinds = {k: (_axis_uniformity(_fold_axes(c, k)[0]), _axis_uniformity(_fold_axes(c, k)[1])) for k in AXES}
    assert kinds['regular'] == ((True, True), (True, True)) and kinds['tables'] == ((True, False), (True, False))
    assert kinds['flags'][0][1] is False and kinds['flags'][1] == (True, True)
    assert _epoch_groups(4, True, True, {}) == [2, 2] and _epoch_groups(4, True, True, {'RAIDER_HIP_EPOCHS_PR_F64_MAX': '4'}) == [4]
    assert _epoch_groups(4, True, False, {}) == [4] and _epoch_groups(2, False, True, {}) == [2]


@pytest.mark.parametrize('case', CASES, ids=[c.id for c in CASES])
def test_between_half_and_95_percent_of_the_reference_is_finite(case):
    for e, ref in enumerate(_reference(case)):
        for w, h, npn in ref:
            fw, fh = np.isfinite(w).mean(), np.isfinite(h).mean()
            assert 0.5 <= fw <= 0.95 and 0.5 <= fh <= 0.95, (case.id, e, fw, fh)
            assert np.array_equal(np.isfinite(w), np.isfinite(h))
    if case.D > 1:                      # the NaN block is in epoch 1 alone
        ref = _reference(case)
        assert all(np.isnan(ref[1][k][0]).sum() > np.isnan(ref[0][k][0]).sum() for k in range(len(ref[0])))
        assert all(np.array_equal(np.isnan(ref[0][k][0]), np.isnan(ref[e][k][0])) for e in range(2, case.D) for k in range(len(ref[0])))


def test_per_pixel_oracle_with_a_model_projection():
    """The addition to the oracle: the per-pixel restatement projects every sample where the slice restatement does.  With equal
    heights it IS the slice oracle with model_proj (bytes); with model_proj=None it is the per-pixel oracle as it was (bytes); and the
    C form agrees with the NumPy one, built from lcc_forward / stere_forward and the pinned slice functions, on mixed heights."""
    case = next(c for c in SINGLE if c.crs == 'lcc' and c.per_ray)
    s = _scene(case)
    c = s['cubes'][0]
    for ht in (0.0, 300.0, float(c['zs'][3])):
        ws, hs, nps = OC.build_cube_ray_slice(c, s['xp'], s['yp'], ht, s['los'], s['zref'], model_proj=LCC)
        w, h, npp = OC.build_cube_ray_per_pixel(c, s['yy'], s['xx'], np.full(s['yy'].shape, ht), s['los'], s['zref'], model_proj=LCC)
        idx = [zz for zz, _, _ in O.ray_levels_idx(c['zs'], ht, s['zref'])]
        assert np.array_equal(npp[idx], nps) and npp.sum() == nps.sum()
        assert w.tobytes() == ws.tobytes() and h.tobytes() == hs.tobytes() and 0.5 < np.isfinite(w).mean() < 0.95
    ll = _scene(next(c for c in SINGLE if c.crs == 'lonlat' and c.per_ray))
    a = OC.build_cube_ray_per_pixel(ll['cubes'][0], ll['yy'], ll['xx'], ll['hts'], ll['los'], ll['zref'])
    b = OC.build_cube_ray_per_pixel(ll['cubes'][0], ll['yy'], ll['xx'], ll['hts'], ll['los'], ll['zref'], model_proj=None)
    assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b))
    # C against NumPy on a few rays with the planted heights among them, Lambert cone; NumPy alone knows the stereographic one
    pick = np.ravel_multi_index(([3, 4, 5, 2, 0, 10, 20, 12], [5, 6, 7, 3, 0, 18, 30, 36]), (NY, NX))
    lat, lon, hts, los = s['yy'].ravel()[pick], s['xx'].ravel()[pick], s['hts'].ravel()[pick], s['los'].reshape(-1, 3)[pick]
    ip = list(O.getInterpolators(c['xs'], c['ys'], c['zs'], c['wet'], c['hydro']))
    wn, hn, npn = O.build_cube_ray_per_pixel(lat, lon, hts, los, ip, MAX_TROPO_HEIGHT=s['zref'], model_proj=LCC)
    wc, hc, npc = OC.build_cube_ray_per_pixel(c, lat, lon, hts, los, s['zref'], model_proj=LCC)
    assert np.array_equal(npn, npc) and np.isfinite(wn).sum() >= 5 and np.isnan(wn).any()
    np.testing.assert_allclose(wc, wn, rtol=0, atol=1e-11, equal_nan=True); np.testing.assert_allclose(hc, hn, rtol=0, atol=1e-11, equal_nan=True)
    with pytest.raises(ValueError, match='Lambert'):
        OC.build_cube_ray_per_pixel(c, lat, lon, hts, los, s['zref'], model_proj=STERE)
    st = _scene(next(c for c in SINGLE if c.crs == 'stere'))
    cs = st['cubes'][0]
    ips = list(O.getInterpolators(cs['xs'], cs['ys'], cs['zs'], cs['wet'], cs['hydro']))
    (rw, rh), rnp = O.build_cube_ray(st['xp'][:6], st['yp'][:4], np.array([300.0]), lambda ht, llh, xyz, yy: st['los'][:4, :6], ips,
                                     MAX_TROPO_HEIGHT=st['zref'], return_nparts=True, model_proj=STERE)
    idx = [zz for zz, _, _ in O.ray_levels_idx(cs['zs'], 300.0, st['zref'])]
    wp, hp, npp = O.build_cube_ray_per_pixel(st['yy'][:4, :6], st['xx'][:4, :6], np.full((4, 6), 300.0), st['los'][:4, :6], ips,
                                             MAX_TROPO_HEIGHT=st['zref'], model_proj=STERE)
    assert np.array_equal(npp[idx], rnp[0]) and np.isfinite(rw).all()
    np.testing.assert_allclose(wp.reshape(4, 6), rw[0], rtol=0, atol=1e-12); np.testing.assert_allclose(hp.reshape(4, 6), rh[0], rtol=0, atol=1e-12)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope='module')
def R():
    import raider_amd
    return raider_amd


def _gpu_cubes(R, s):
    cubes = [R.Cube(c['ys'], c['xs'], c['zs'], c['wet'], c['hydro'], order='zyx') for c in s['cubes']]
    p = s['proj']
    for cb in cubes:
        if p is not None and p.get('proj') == 'stere':
            cb.set_projection_stere(**{k: v for k, v in p.items() if k != 'proj'})
        elif p is not None:
            cb.set_projection_lcc(**p)
    return cubes


def _gpu_rays(R, s, form, ht):
    """the batch of one slice height ht, or of the per-ray heights (ht None); stacked slices share one batch (ht: their heights)"""
    hts = s['hts']
    kw = {} if hts is None else dict(hts=hts)
    kwp = {} if hts is None else dict(hts=hts.ravel())
    if form == 'grid_los':
        return R.Rays.grid(s['xp'], s['yp'], los=s['los'], **kw)
    if form == 'grid_inc':
        return R.Rays.grid(s['xp'], s['yp'], inc=s['inc'], hd=s['hd'], **kw)               # (a heading RASTER)
    if form == 'llh_los':
        return R.Rays.points(lat=s['yy'].ravel(), lon=s['xx'].ravel(), los=s['los'].reshape(-1, 3), **kwp)
    if form == 'xyz_los':
        xyz = np.stack(O.lla2ecef(s['yy'].ravel(), s['xx'].ravel(), hts.ravel() if hts is not None else np.full(NY * NX, float(ht))), -1)
        return R.Rays.points(xyz=np.ascontiguousarray(xyz), los=s['los'].reshape(-1, 3), **kwp)   # (no lat / lon: the kernel finds the frame)
    raise KeyError(form)


def _gpu_reached(R, case, cubes, rays, n_generic, n_active):
    """the model applied to the objects the library was handed"""
    from raider_amd import _lib as L
    cb = cubes[0]
    assert all(c.dtype == cb.dtype and c.projection == cb.projection for c in cubes)
    return _reached(cb.dtype == np.float64, cb.projection, cb.grid[0], cb.grid[1], rays.struct.origin_mode == L.ORIGIN_GRID,
                    rays.struct.los_mode == L.LOS_VEC, rays.ht_min is not None, len(cubes), n_generic, n_active, os.environ)


def _assert_reached(R, case, cubes, rays, n_active):
    n_generic = cubes[0].ctx.generic_ray_count()
    got = _gpu_reached(R, case, cubes, rays, n_generic, n_active)
    assert got == case.want, f'{case.id} is named for {sorted(case.want)} and reaches {sorted(got)}'


def _against(case, what, w, h, npn, ref, worst):
    ow, oh, onp = ref
    assert np.array_equal(npn, onp), (case.id, what, npn, onp)
    w, h = np.asarray(w).reshape(ow.shape), np.asarray(h).reshape(oh.shape)
    assert np.array_equal(np.isnan(w), np.isnan(ow)) and np.array_equal(np.isnan(h), np.isnan(oh)), (case.id, what, 'NaN mask')
    dw, dh = np.nanmax(np.abs(w - ow)), np.nanmax(np.abs(h - oh))
    worst[0] = max(worst[0], dw); worst[1] = max(worst[1], dh)
    assert dw <= TOL and dh <= TOL, (case.id, what, dw, dh, np.unravel_index(np.nanargmax(np.abs(h - oh)), oh.shape))


def _pr_nparts(cube, rays, zref, onp):
    """the oracle's partition by model interval, on the levels of the table built for the lowest ray (test_gpu_perpixel.py: _oracle_vs_gpu)"""
    kz = cube.ray_levels(rays.ht_min, zref)[2]
    assert not onp[np.setdiff1d(np.arange(onp.size), kz)].any()
    return onp[kz]


@pytest.mark.gpu
@pytest.mark.parametrize('case', SINGLE, ids=[c.id for c in SINGLE])
def test_single_cube_instantiation_against_the_oracle(R, case):
    s = _scene(case)
    ref = _reference(case)[0]
    (cube,) = cubes = _gpu_cubes(R, s)
    worst = [0.0, 0.0]
    if case.per_ray:
        rays = _gpu_rays(R, s, case.form, None)
        w, h, npn, fl = cube.raytrace(rays, None, s['zref'])
        _assert_reached(R, case, cubes, rays, NY * NX)
        ow, oh, onp = ref[0]
        _against(case, 'per-ray heights', w, h, npn, (ow, oh, _pr_nparts(cube, rays, s['zref'], onp)), worst)
    else:
        got = []
        for ht in s['heights']:
            rays = _gpu_rays(R, s, case.form, ht)
            got.append(cube.raytrace(rays, ht, s['zref']))
            _assert_reached(R, case, cubes, rays, NY * NX)          # (before any delay is looked at)
        for ht, (w, h, npn, fl), r in zip(s['heights'], got, ref):
            _against(case, f'slice {ht}', w, h, npn, r, worst)
    print(f'RAYINST {case.id} {" ".join(sorted(case.want))} wet {worst[0]:.2e} hydro {worst[1]:.2e}')


@pytest.mark.gpu
@pytest.mark.parametrize('case', STACKED, ids=[c.id for c in STACKED])
def test_stacked_instantiation_against_the_oracle_in_every_epoch(R, case, monkeypatch):
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)                                   # (epoch_group reads it per call)
    s = _scene(case)
    ref = _reference(case)
    cubes = _gpu_cubes(R, s)
    worst = [0.0, 0.0]
    if case.per_ray:
        rays = _gpu_rays(R, s, case.form, None)
        w, h, npn, fl = R.raytrace_epochs(cubes, rays, None, s['zref'])
        _assert_reached(R, case, cubes, rays, NY * NX)
        assert w.shape[0] == case.D
        for e in range(case.D):
            ow, oh, onp = ref[e][0]
            _against(case, f'epoch {e}', w[e], h[e], npn, (ow, oh, _pr_nparts(cubes[0], rays, s['zref'], onp)), worst)
    else:
        rays = _gpu_rays(R, s, case.form, None)
        w, h, K, npt, fl = R.raytrace_slices_epochs(cubes, rays, list(s['heights']), s['zref'])
        _assert_reached(R, case, cubes, rays, NY * NX * len(s['heights']))
        assert w.shape[:2] == (case.D, len(s['heights']))
        for e in range(case.D):
            for k, ht in enumerate(s['heights']):
                _against(case, f'epoch {e} slice {ht}', w[e, k], h[e, k], npt[k, :K[k]], ref[e][k], worst)
    assert not np.array_equal(w[0], w[1], equal_nan=True)
    print(f'RAYINST {case.id} {" ".join(sorted(case.want))} wet {worst[0]:.2e} hydro {worst[1]:.2e}')
