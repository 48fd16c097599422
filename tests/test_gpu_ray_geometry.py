"""The light ray geometry on the device against a model of its design (tests/ray_poly_model.py).

The delay-level suites see the ray polynomials only through smooth synthetic fields, which attenuate a horizontal position error by
about 1e-9 per metre, and through nParts = ceil(maxlen / 1000) + 1.  Here the geometry itself is compared:

  a. the level length maxima of pass 1 (Cube.ray_prepass) with the model's, level by level, at the rounding level of the node
     geodesy: 2 (Lebesgue constant of six Chebyshev nodes) x 2 (crossings per length) x 3e-8 m (height noise of the one-step
     reciprocal square root) / cos(largest incidence);
  b. the sample positions of pass 2 through cubes that are LINEAR in one coordinate (trilinear interpolation of a linear field is the
     field, so a delay is the path integral of the coordinate polynomial): the difference to the model's trapezoid sum, as a
     path-mean position in metres, within 4 x the distance of the two CPU restatements of the reference on the same cube;
  c. on the high-latitude scenes, where the interpolation error of the design is largest, what that error does to a delay under the
     strongest horizontal gradient of the synthetic weather cube - apart from what the offset of the level crossings against the
     reference's height does on the same cube.  The first part is what the longitude-travel limit of the classification is set by.

Measured on an MI355X: maxima within 4e-9 m of the model's (tolerance 1.9e-7 m, 3.5e-7 m at 70 degrees); positions within 4.4e-8 m
(lat, lon) and 3.4e-9 m (h) as a path mean - 0.9 .. 3.6 of the CPU floor.  The model's polynomials sit 3e-10 .. 7e-10 m (lat, lon) from
the reference's geodesy on the mid-latitude scenes as a path mean, 3e-7 .. 2.5e-6 m on the high-latitude ones, 2e-6 .. 3e-6 m in h
(the reference's own height formula).  Seeded in scratch builds (with the longitude-travel limit at 0.2 rad and the H scenes at
78-82 deg N, before the limit was tightened to 0.12 rad): asin_small without its s^7 term failed H1-lon and H2-lon alone (2e-3 m at
H2) and no delay-level case - at 0.12 rad it still fails H2-lon (4e-4 m) and the H2 delay impact, and no delay-level case; one entry
of RAY_POLY_VINV changed in its 6th digit, or the bare reciprocal-square-root seed throughout
geo_fast<true>, failed 36 of the 38 cases here (and the delay-level suites too: 2e-6 m of delay); the bare seed in the first stage of
the node latitude alone moved latitudes by 3e-4 .. 7e-4 m and failed every latitude case, where 8 of 68 delay-level cases saw
1.4e-9 .. 7e-9 m.

Scenes: 21 x 37 rays (partial 16 x 16 tiles both ways), 40 x 44 x 24 cubes whose hull contains every sample (a CPU test).
Every GPU case prints `RAYGEOM <scene> <generic rays> <max |gpu - model|> <max |model - oracle|>`, the latter in its two parts."""
from collections import namedtuple

import numpy as np
import pytest

from oracle import raider_oracle as O
from oracle import oracle_c as OC
from tests import ray_poly_model as M
from tests.test_gpu_ray_instantiations import LCC, NX, NY, _generic_rays, _gpu_rays, _heights
from tests.test_ray_poly_bounds import BOUND_CROSSING, BOUND_LAT, BOUND_LON

CUBE = (40, 44, 24)
TIGHT = 1e-9                        # tests/test_gpu_parity.py
NODE_NOISE = 3e-8                   # metres of height at a fit node (one Newton-Raphson step, 4e-15 of 6.4e6 m)
LEBESGUE6 = 2.0                     # (the Lebesgue constant of 6 Chebyshev nodes is 1.99)

# cube: (y0, y1, x0, x1, ztop) of O.synthetic_cube; rays: ((lon a, lon b), (lat a, lat b)); inc: (lo, hi) ramp across the scene
Scene = namedtuple('Scene', 'cube rays inc hd heights per_ray proj generic')
SCENES = {
    'M': Scene((30.0, 36.0, -121.0, -113.0, 41000.0), ((-119.5, -114.5), (35.0, 31.0)), (20.0, 50.0), -167.9, (0.0, 300.0), False, None, False),
    'S': Scene((29.0, 36.0, -121.0, -113.0, 41000.0), ((-119.5, -114.5), (35.0, 31.0)), (55.0, 70.0), -167.9, (0.0, 300.0), False, None, False),
    'H1': Scene((73.0, 81.0, -124.0, -103.0, 41000.0), ((-119.5, -114.5), (79.5, 75.5)), (55.0, 70.0), -167.9, (0.0, 300.0), False, None, False),
    'H2': Scene((73.0, 81.0, -124.0, -103.0, 41000.0), ((-119.5, -114.5), (79.5, 75.5)), (55.0, 70.0), -90.0, (0.0, 300.0), False, None, False),
    'P': Scene((30.0, 36.0, -121.0, -113.0, 41000.0), ((-119.5, -114.5), (35.0, 31.0)), (20.0, 50.0), -167.9, None, True, None, False),
    'L': Scene((-9.0e5 + LCC['y_0'], 1.0e5 + LCC['y_0'], -2.2e6 + LCC['x_0'], -1.3e6 + LCC['x_0'], 41000.0), ((-119.0, -114.0), (36.5, 33.0)),
               (20.0, 50.0), -167.9, (0.0, 300.0), False, LCC, False),
    'G': Scene((86.0, 89.9, -60.0, 60.0, 15000.0), ((-25.0, 25.0), (89.5, 88.95)), (20.0, 50.0), -167.9, (9300.0, 9800.0), False, None, True),
}
LIGHT = [k for k, v in SCENES.items() if not v.generic]

_memo = {}


def _once(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def _scene(name):
    """everything a case hands to the library, the oracle and the model (the dict _gpu_rays of test_gpu_ray_instantiations reads)"""
    def build():
        sc = SCENES[name]
        ny, nx, nz = CUBE
        y0, y1, x0, x1, ztop = sc.cube
        c = O.synthetic_cube(ny, nx, nz, seed=8, ztop=ztop, y0=y0, y1=y1, x0=x0, x1=x1)
        (xa, xb), (ya, yb) = sc.rays
        xp, yp = np.linspace(xa, xb, NX), np.linspace(ya, yb, NY)
        xx, yy = np.meshgrid(xp, yp)
        inc = np.broadcast_to(sc.inc[0] + (sc.inc[1] - sc.inc[0]) * np.arange(NX) / (NX - 1), (NY, NX)).copy()
        los = np.ascontiguousarray(O.look_vectors_from_inc_hd(inc, np.full((NY, NX), sc.hd), yy, xx, 0.0))
        return dict(c=c, proj=sc.proj, xp=xp, yp=yp, xx=xx, yy=yy, inc=inc, los=los, zref=float(c['zs'].max() - 1), heights=sc.heights,
                    hts=_heights(c['zs']) if sc.per_ray else None, cos_min=float(np.cos(np.radians(sc.inc[1]))))
    return _once(('scene', name), build)


def _slices(s):
    """[(ht handed to the library, heights handed to the model)]"""
    return [(None, s['hts'])] if s['hts'] is not None else [(ht, ht) for ht in s['heights']]


def _frame(s, form, hts):
    """lat, lon, ECEF origins as the kernel sees them for this origin form"""
    if form != 'xyz_los':
        return s['yy'], s['xx'], None
    xyz = np.stack(O.lla2ecef(s['yy'].ravel(), s['xx'].ravel(), np.broadcast_to(hts, s['yy'].shape).ravel()), -1)
    lon, lat, _ = O.ecef2lla(xyz[:, 0], xyz[:, 1], xyz[:, 2])               # (no lat / lon in the batch: the kernel finds the frame)
    return lat, lon, xyz


def _model(name, form='grid_los'):
    """per slice: (q, crossings, maxlen) of the model"""
    def build():
        s = _scene(name)
        out = []
        for ht, hts in _slices(s):
            lat, lon, xyz = _frame(s, form, hts)
            q = M.fit(lat, lon, s['los'], hts, s['zref'], proj=s['proj'], xyz=xyz)
            cr = M.crossings(q, s['c']['zs'], float(np.min(hts)), s['zref'], per_ray=ht is None)
            out.append((q, cr, M.maxlen(cr)))
        return out
    return _once(('model', name, 'xyz' if form == 'xyz_los' else 'llh'), build)


def _oracle_prepass(name):
    """per slice: (maxlen on the levels of the library's table, clamp pair) from the C oracle"""
    def build():
        s = _scene(name)
        out = []
        for ht, hts in _slices(s):
            if ht is None:
                ml, clamp = OC.per_pixel_prepass(s['c'], s['yy'], s['xx'], hts, s['los'], s['zref'])
                ml = ml[M.level_table(s['c']['zs'], float(hts.min()), s['zref'])[2]]
            else:
                ml, clamp = OC.ray_prepass(s['c'], s['xp'], s['yp'], ht, s['los'], s['zref'])
            out.append((ml, clamp))
        return out
    return _once(('oracle', name), build)


def _flags_of(clamp):
    """the oracle's clamp pair as pass 1 reports it: 2 = some finite length, 4 / 8 = NOT every first / last sample outside the cube"""
    return 2 | (0 if clamp[0] else 4) | (0 if clamp[1] else 8)


def _generic_count(s):
    return sum(_generic_rays(s['proj'], s['c']['xs'], s['yy'], s['xx'], s['los'], hts, s['zref']) for _, hts in _slices(s))


# ---- linear cubes --------------------------------------------------------------------------------------------------------------------
# field name -> (coordinate polynomial of the model, cube axis it is linear in, metres of position per unit of the field)
FIELDS = ('lat', 'lon', 'h')
H_MID, H_UNIT, LCC_UNIT = 20000.0, 1000.0, 1e-5
PP_STRIDE = 37


def _centre(s, field):
    if s['proj'] is not None and field != 'h':
        x, y = O.lcc_forward(s['yy'].mean(), s['xx'].mean(), **s['proj'])
        return float(y if field == 'lat' else x)
    return dict(lat=float(s['yy'].mean()), lon=float(s['xx'].mean()), h=H_MID)[field]


def _unit(s, field):
    """(what the cube holds per unit of the coordinate, metres on the ground per unit of the coordinate)"""
    if field == 'h':
        return 1.0 / H_UNIT, 1.0
    if s['proj'] is not None:
        return LCC_UNIT, 1.0
    return 1.0, 111e3 * (np.cos(np.radians(np.abs(s['yy']).max())) if field == 'lon' else 1.0)


def _linear_cube(s, field, factor=1.0):
    """f64 cube whose wet AND hydro fields are factor * (coordinate - centre) * unit"""
    c = s['c']
    shape = (c['zs'].size, c['ys'].size, c['xs'].size)
    ax = dict(lat=c['ys'][None, :, None], lon=c['xs'][None, None, :], h=c['zs'][:, None, None])[field]
    v = np.ascontiguousarray(np.broadcast_to(factor * _unit(s, field)[0] * (ax - _centre(s, field)), shape), dtype=np.float64)
    return dict(ys=c['ys'], xs=c['xs'], zs=c['zs'], wet=v, hydro=v.copy())


def _oracle_delays(name, field, factor=1.0):
    """per slice: (C oracle's delay, NumPy oracle's delay, nParts of the table's levels, clamp pair) on the linear cube"""
    def build():
        s = _scene(name)
        c = _linear_cube(s, field, factor)
        ip = list(O.getInterpolators(c['xs'], c['ys'], c['zs'], c['wet'], c['hydro']))
        out = []
        for (ht, hts), (_, clamp) in zip(_slices(s), _oracle_prepass(name)):
            if ht is None:
                w, _, npn = OC.build_cube_ray_per_pixel(c, s['yy'], s['xx'], hts, s['los'], s['zref'], model_proj=s['proj'])
                # the NumPy form goes ray by ray: every PP_STRIDE-th ray and the planted heights, with the batch's partition (the other rays
                # stay out of the floor, which can only lower it)
                pick = np.union1d(np.arange(0, NY * NX, PP_STRIDE), np.ravel_multi_index(([3, 4, 5, 2], [5, 6, 7, 3]), (NY, NX)))
                wp = O.build_cube_ray_per_pixel(s['yy'].ravel()[pick], s['xx'].ravel()[pick], hts.ravel()[pick], s['los'].reshape(-1, 3)[pick], ip,
                                                MAX_TROPO_HEIGHT=s['zref'], nParts_override=npn, model_proj=s['proj'])[0]
                wn = w.copy(); wn.ravel()[pick] = wp
                npn = npn[M.level_table(c['zs'], float(hts.min()), s['zref'])[2]]
            else:
                w, _, npn = OC.build_cube_ray_slice(c, s['xp'], s['yp'], ht, s['los'], s['zref'], model_proj=s['proj'])
                (wn, _), nps = O.build_cube_ray(s['xp'], s['yp'], np.array([ht]), lambda *a: s['los'], ip, MAX_TROPO_HEIGHT=s['zref'],
                                                return_nparts=True, model_proj=s['proj'])
                assert np.array_equal(nps[0], npn)
                wn = wn[0]
            out.append((w, wn, np.asarray(npn), clamp))
        return out
    return _once(('delays', name, field, factor), build)


def _model_delays(name, field, factor=1.0):
    """per slice: (model's delay [NY, NX], sum of the lengths) with the oracle's partition"""
    def build():
        s = _scene(name)
        out = []
        for (q, cr, _), (_, _, npn, _) in zip(_model(name), _oracle_delays(name, field, factor)):
            d, ls = M.linear_field_delay(q, cr, npn, field, _centre(s, field), factor * _unit(s, field)[0])
            out.append((d.astype(np.float64).reshape(NY, NX), ls.astype(np.float64).reshape(NY, NX)))
        return out
    return _once(('mdelays', name, field, factor), build)


def _reference_coord(s, field, q, us):
    """the reference's geodesy (raider_oracle.ecef2lla, lcc_forward on a cone) at the model's own sample points"""
    x, y, z = (v.astype(np.float64) for v in M.sample_points(q, us))
    lon, lat, h = O.ecef2lla(x, y, z)
    if field == 'h':
        return h
    if s['proj'] is not None:
        px, py = O.lcc_forward(lat, lon, **s['proj'])
        return py if field == 'lat' else px
    return lat if field == 'lat' else lon


def _strongest_gradient(s, field, by_level=False):
    """largest horizontal difference quotient of the synthetic weather cube's refractivity (wet + hydro), N-units per degree; by_level:
    per model level [nz]"""
    c = s['c']
    n = c['wet'].astype(np.float64) + c['hydro'].astype(np.float64)
    ax, g = (1, c['ys']) if field == 'lat' else (2, c['xs'])
    d = np.abs(np.diff(n, axis=ax)).max(axis=(1, 2)) / np.abs(np.diff(g)).min()
    return d if by_level else float(d.max())


def _hybrid_delays(name, field, factor=1.0):
    """What splits |model - oracle| into its two causes.  Per slice a dict:
      hybrid   the model's crossings and partition with the REFERENCE's geodesy at the samples.  model - hybrid is the interpolation
               error of the coordinate polynomial alone (what the static classification governs); hybrid - oracle is what the offset of
               the crossings does (the kernels' exact height against the reference's p / cos(phi) - N: 1.7e-5 m at 40 km, whatever
               the classification) - it moves the ends of the path, so it goes with the field's VALUE at the top, not with its gradient
      ends     |field| at the ray's first and last sample, summed (bounds the second)
      weather  lat / lon on a lon/lat cube: the interpolation part when the gradient follows the synthetic cube's own strongest
               gradient at each height (N-units per degree, interpolated between the model levels) instead of one value held
               through the column"""
    def build():
        s = _scene(name)
        centre, unit = _centre(s, field), factor * _unit(s, field)[0]
        gz = _strongest_gradient(s, field, by_level=True) if field != 'h' and s['proj'] is None else None
        out = []
        for (q, cr, _), (_, _, npn, _) in zip(_model(name), _oracle_delays(name, field, factor)):
            hyb = M.path_sum(q, cr, npn, lambda us: unit * (_reference_coord(s, field, q, us) - centre))
            first = cr['u'][np.arange(cr['k0'].size), cr['k0']]
            ends = sum(np.abs(unit * (_reference_coord(s, field, q, u[:, None])[:, 0] - centre)) for u in (first, cr['u'][:, -1]))
            d = dict(hybrid=hyb.astype(np.float64).reshape(NY, NX), ends=ends.reshape(NY, NX), cosi=q['cosi'].astype(np.float64).reshape(NY, NX))
            if gz is not None:
                def integrand(us):
                    hh = _reference_coord(s, 'h', q, us)
                    return np.interp(hh, s['c']['zs'], gz) * (M.polyval(q[field], us).astype(np.float64) - _reference_coord(s, field, q, us))
                d['weather'] = M.path_sum(q, cr, npn, integrand).astype(np.float64).reshape(NY, NX)
            out.append(d)
        return out
    return _once(('hybrid', name, field, factor), build)


def _position(s, field, delta, lengths):
    """a delay difference on a linear cube as a path-mean position difference in metres"""
    cube_unit, metres = _unit(s, field)
    return np.abs(delta) / (1e-6 * lengths) / cube_unit * metres


# ---- CPU: the scenes are what the GPU cases take them for ------------------------------------------------------------------------------


@pytest.mark.parametrize('name', list(SCENES))
def test_scene_is_inside_its_cube_and_classified_as_named(name):
    s = _scene(name)
    n = _generic_count(s)
    assert n == (NY * NX * len(_slices(s)) if SCENES[name].generic else 0), (name, n)
    assert n == sum(int((~M.classify(s['yy'], s['xx'], s['los'], hts, s['zref'], s['proj'], s['c']['xs'])).sum()) for _, hts in _slices(s))
    for ht, hts in _slices(s):
        if ht is None:
            w, h, _ = OC.build_cube_ray_per_pixel(s['c'], s['yy'], s['xx'], hts, s['los'], s['zref'], model_proj=s['proj'])
        else:
            w, h, _ = OC.build_cube_ray_slice(s['c'], s['xp'], s['yp'], ht, s['los'], s['zref'], model_proj=s['proj'])
        assert np.isfinite(w).all() and np.isfinite(h).all(), (name, ht, np.isfinite(w).mean())


@pytest.mark.parametrize('name', LIGHT)
def test_model_against_the_oracle_on_the_scenes(name):
    """The model is the yardstick of the GPU cases; its own distance to the reference is the design error DESIGN.md B.3 documents and
    tests/test_ray_poly_bounds.py pins: crossings within 2e-5 m of height, hence lengths within 2 x 2e-5 m / cos(inc)."""
    s = _scene(name)
    crossing = BOUND_CROSSING[40000.0]                  # (the scenes' 41 km top: 1.67e-5 m at 40 km grows with the square of the height)
    for (q, cr, ml), (oml, clamp) in zip(_model(name), _oracle_prepass(name)):
        assert ml.shape == oml.shape and np.abs(ml - oml).max() <= 2 * crossing / s['cos_min'], (name, np.abs(ml - oml).max())
        assert clamp == (0, 0)
    for field in FIELDS:
        for (w, wn, npn, _), (d, ls), hy in zip(_oracle_delays(name, field), _model_delays(name, field), _hybrid_delays(name, field)):
            assert np.isfinite(w).all() and np.isfinite(d).all() and np.isfinite(hy['hybrid']).all()
            # the interpolation part as a path-mean position: the bounds of B.3 over every admitted ray (h: the fit against the
            # reference's height, which is itself up to 1.7e-5 m off the exact one at the top)
            pos = _position(s, field, d - hy['hybrid'], ls).max()
            assert pos <= dict(h=crossing, lat=BOUND_LAT[0], lon=BOUND_LON[0])[field], (name, field, pos)
            # the crossing part: the two ends of the path move by at most `crossing` of height, 1 / cos(inc) of that along the ray
            assert (np.abs(hy['hybrid'] - w) <= 1e-6 * hy['ends'] * crossing / hy['cosi']).all(), (name, field, np.abs(hy['hybrid'] - w).max())


@pytest.mark.parametrize('name', [n for n in LIGHT if SCENES[n].proj is None])
def test_delay_impact_split_into_its_two_causes(name):
    """The linear cubes scaled to the strongest horizontal refractivity gradient of the synthetic cube, held through the whole column
    (test_delay_impact_of_the_design_error_at_high_latitude runs them on the device): |model - oracle| in metres of delay, split into
    the interpolation part and the crossing part (_hybrid_delays), printed for every scene so that the figures of DESIGN.md B.3 can be
    reproduced.  Asserted: each part within what the bounds of tests/test_ray_poly_bounds.py allow a ray."""
    s = _scene(name)
    crossing = BOUND_CROSSING[40000.0]
    for field in ('lat', 'lon'):
        g = _strongest_gradient(s, field)
        per_degree = 111e3 * (np.cos(np.radians(s['yy'])) if field == 'lon' else 1.0)
        tot = fit = cro = wea = 0.0
        for (w, _, _, _), (d, ls), hy in zip(_oracle_delays(name, field, g), _model_delays(name, field, g), _hybrid_delays(name, field, g)):
            tot, fit, cro = max(tot, np.abs(d - w).max()), max(fit, np.abs(d - hy['hybrid']).max()), max(cro, np.abs(hy['hybrid'] - w).max())
            wea = max(wea, np.abs(_hybrid_delays(name, field)[0]['weather']).max())
            assert (np.abs(d - hy['hybrid']) <= g * (BOUND_LAT if field == 'lat' else BOUND_LON)[0] / per_degree * 1e-6 * ls).all()
            assert (np.abs(hy['hybrid'] - w) <= 1e-6 * hy['ends'] * crossing / hy['cosi']).all()
        print(f'RAYGEOM {name} delay impact by the model, {field} gradient {g:.1f} N/deg held through the column: |model - oracle| {tot:.2e} m = '
              f'interpolation {fit:.2e} m, crossing offset {cro:.2e} m; interpolation with the cube\'s gradient at each height {wea:.2e} m')
        assert fit <= TIGHT, (name, field, g, fit)              # (what the longitude-travel limit of the classification is set by)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope='module')
def R():
    import raider_amd
    return raider_amd


def _gpu_cube(R, c, proj, dtype):
    cube = R.Cube(c['ys'], c['xs'], c['zs'], c['wet'].astype(dtype), c['hydro'].astype(dtype), order='zyx')
    if proj is not None:
        cube.set_projection_lcc(**proj)
    return cube


def _rays(R, s, form, ht):
    return _gpu_rays(R, s, form, ht)


PREPASS = ([(n, f64, 'grid_los') for n in SCENES for f64 in (False, True)]
           + [('M', True, 'llh_los'), ('M', False, 'xyz_los'), ('P', True, 'xyz_los'), ('L', False, 'llh_los')])


@pytest.mark.gpu
@pytest.mark.parametrize('name,f64,form', PREPASS, ids=[f'{n}-{"f64" if d else "f32"}-{f}' for n, d, f in PREPASS])
def test_level_length_maxima_against_the_model(R, name, f64, form):
    s = _scene(name)
    cube = _gpu_cube(R, s['c'], s['proj'], np.float64 if f64 else np.float32)
    tol = 2 * LEBESGUE6 * NODE_NOISE / s['cos_min']
    worst, worst_mo, generic = 0.0, 0.0, 0
    got = []
    for ht, hts in _slices(s):
        got.append(cube.ray_prepass(_rays(R, s, form, ht), ht, s['zref']))
        generic += cube.ctx.generic_ray_count()
    assert generic == (NY * NX * len(got) if SCENES[name].generic else 0), (name, generic)
    if SCENES[name].generic:
        # the generic kernels run the reference's own Newton iteration on the reference's height: the oracle is the yardstick, at the
        # distance of two CPU implementations of that one algorithm
        for (ht, hts), (ml, fl), (oml, clamp) in zip(_slices(s), got, _oracle_prepass(name)):
            xyz = np.stack(O.lla2ecef(s['yy'], s['xx'], ht), -1)
            rl = O.build_ray(s['c']['zs'], ht, xyz, s['los'], s['zref'])[0]
            floor = np.abs(rl.reshape(oml.size, -1).max(1) - oml).max()
            d = np.abs(ml - oml).max()
            print(f'RAYGEOM {name} generic {generic} gpu-oracle {d:.2e} floor {floor:.2e}')
            assert floor > 0 and d <= 4 * floor, (name, ht, d, floor)
            assert fl == _flags_of(clamp), (name, ht, fl, clamp)
        return
    for (ml, fl), (q, cr, mml), (oml, clamp) in zip(got, _model(name, form), _oracle_prepass(name)):
        assert ml.shape == mml.shape == oml.shape
        d, mo = np.abs(ml - mml), np.abs(mml - oml)
        worst, worst_mo = max(worst, d.max()), max(worst_mo, mo.max())
        print(f'RAYGEOM {name} generic {generic} gpu-model {d.max():.2e} model-oracle {mo.max():.2e} (maxlen, m; tolerance {tol:.2e})')
        assert (d <= tol).all(), (name, form, d.max(), tol, int(d.argmax()))
        assert (np.abs(ml - oml) <= mo + tol).all(), (name, form, np.abs(ml - oml).max())
        assert fl == _flags_of(clamp), (name, fl, clamp)


MARCH = [(n, f) for n in LIGHT for f in FIELDS]


@pytest.mark.gpu
@pytest.mark.parametrize('name,field', MARCH, ids=[f'{n}-{f}' for n, f in MARCH])
def test_sample_positions_through_linear_cubes(R, name, field):
    s = _scene(name)
    cube = _gpu_cube(R, _linear_cube(s, field), s['proj'], np.float64)
    form = 'llh_los' if name == 'L' and field == 'lon' else 'grid_los'            # (per-ray cone origins once)
    for (ht, hts), (w, wn, npn, clamp), (d, ls), hy in zip(_slices(s), _oracle_delays(name, field), _model_delays(name, field),
                                                         _hybrid_delays(name, field)):
        gw, gh = cube.ray_march(_rays(R, s, form, ht), ht, s['zref'], npn, _flags_of(clamp))
        generic = cube.ctx.generic_ray_count()
        gw, gh = np.asarray(gw).reshape(NY, NX), np.asarray(gh).reshape(NY, NX)
        assert generic == 0 and np.isfinite(gw).all() and np.array_equal(gw, gh)
        floor = _position(s, field, wn - w, ls).max()
        # (model - oracle in its two parts, _hybrid_delays: the polynomial against the reference's geodesy at the model's samples, and
        # what the offset of the crossings does to this cube's delay - the latter is no position error, it is quoted in the same unit)
        gm, mo, co = _position(s, field, gw - d, ls), _position(s, field, d - hy['hybrid'], ls), _position(s, field, hy['hybrid'] - w, ls)
        print(f'RAYGEOM {name} generic {generic} gpu-model {gm.max():.2e} model-oracle {mo.max():.2e} (interpolation) + {co.max():.2e} (crossing '
              f'offset) ({field}, path-mean m; floor {floor:.2e}; delays to {np.abs(gw).max():.2g} m)')
        assert floor > 0 and gm.max() <= 4 * floor, (name, field, ht, gm.max(), floor, np.unravel_index(gm.argmax(), gm.shape))


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['H1', 'H2'])
def test_delay_impact_of_the_design_error_at_high_latitude(R, name):
    """What the design error of the ray polynomials does to a delay (issue of the longitude-travel limit): the linear cubes scaled to
    the strongest horizontal refractivity gradient of the synthetic cube (N-units per degree, by finite differences), held through the
    WHOLE column up to 41 km.  |gpu - oracle| has two causes, measured apart (_hybrid_delays):
      the interpolation part, gpu - (model crossings + reference geodesy at the samples): what the static classification governs.
        It must stay within the parity bound TIGHT = 1e-9 m; that is what set the limit to 0.12 rad (8.8e-10 m at H1, longitude;
        3.9e-9 m on the same construction at 78-82 deg N under the former 0.2 rad).  It is also the model's, to rounding;
      the crossing part: the kernels' exact height against the reference's p / cos(phi) - N (1.7e-5 m at 40 km) moves the top end of
        the path, so it goes with the field's VALUE there - hundreds of N-units on these cubes, where a weather field has none left
        at 41 km.  4e-9 .. 1e-8 m on every scene, mid-latitude ones alike (test_delay_impact_split_into_its_two_causes prints them);
        independent of the classification, bounded on the CPU."""
    s = _scene(name)
    for field in ('lat', 'lon'):
        g = _strongest_gradient(s, field)
        cube = _gpu_cube(R, _linear_cube(s, field, g), s['proj'], np.float64)
        per_degree = 111e3 * (np.cos(np.radians(s['yy'])) if field == 'lon' else 1.0)
        tot = fit = cro = 0.0
        for (ht, hts), (w, wn, npn, clamp), (d, ls), hy in zip(_slices(s), _oracle_delays(name, field, g), _model_delays(name, field, g),
                                                             _hybrid_delays(name, field, g)):
            gw, _ = cube.ray_march(_rays(R, s, 'grid_los', ht), ht, s['zref'], npn, _flags_of(clamp))
            gw = np.asarray(gw).reshape(NY, NX)
            gfit = gw - hy['hybrid']                   # the device's interpolation part
            tot, fit, cro = max(tot, np.abs(gw - w).max()), max(fit, np.abs(gfit).max()), max(cro, np.abs(hy['hybrid'] - w).max())
            # the device's interpolation part IS the model's, to the rounding of this cube's two CPU oracles ...
            floor = np.abs(wn - w).max()
            assert floor > 0 and np.abs(gfit - (d - hy['hybrid'])).max() <= 4 * floor, (name, field, np.abs(gfit - (d - hy['hybrid'])).max(), floor)
            # ... and within what the position bounds of tests/test_ray_poly_bounds.py allow a ray
            assert (np.abs(gfit) <= g * (BOUND_LAT if field == 'lat' else BOUND_LON)[0] / per_degree * 1e-6 * ls).all(), (name, field, np.abs(gfit).max())
        print(f'RAYGEOM {name} delay impact: {field} gradient {g:.1f} N/deg, |gpu - oracle| {tot:.2e} m = interpolation {fit:.2e} m, '
              f'crossing offset {cro:.2e} m (parity bound {TIGHT:.0e} m)')
        assert fit <= TIGHT, (name, field, g, fit)
