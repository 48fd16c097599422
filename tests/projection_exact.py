"""The map projections of the delay path as their DEFINING equations, evaluated with 40 significant digits (mpmath) - the yardstick of
tests/test_geodesy_exact.py (the oracle, no GPU) and tests/test_gpu_projection_exact.py (tm_kernel / cone_kernel).  Not a test module.

Transverse Mercator needs no series and no coefficients: it is the analytic continuation of the meridian distance M as a function of the
isometric latitude psi,

    psi(p) = asinh(tan p) - e atanh(e sin p)
    M(P)   = a (1 - e^2) int_0^P (1 - e^2 sin^2 t)^(-3/2) dt              (P complex: the integral runs along the straight line 0 .. P)
    w      = psi(phi) + i lam,          lam = lon - lon_0 wrapped to (-pi, pi]
    psi(P) = w                          solved for the complex latitude P by Newton from the spherical answer asin(tanh w)
    z      = k_0 (M(P) - M(lat_0)),     x = x_0 + Im z,   y = y_0 + Re z

(at phi = +-90, where psi is infinite: x = x_0, y = y_0 + k_0 (+-M(pi/2) - M(lat_0))).  Nothing here shares a formula with Krueger's series
(csrc/proj_kernels.h, oracle.raider_oracle.tm_forward).  The cones are Snyder's closed forms (USGS PP 1395: 15-1 .. 15-4, 21-33 / 21-34 /
21-39), which ARE the definition of those projections.

(Checked against the closed form M = a (E(P | e^2) - e^2 sin P cos P / sqrt(1 - e^2 sin^2 P)) with mpmath's incomplete elliptic integral of a
complex argument: equal to 2e-35 m.  It gives 9 997 964.943 020 998 m for the UTM northing of the pole.)

    tm_exact(lat, lon, **params)  /  lcc_exact(lat, lon, **params)  /  stere_exact(lat, lon, **params)   -> (x, y) as mpf
    deviation(x, y, exact)        -> [n] float: max(|x - ex|, |y - ey|) of doubles against exact pairs, in metres
    TM / tm_sets()                -> the parameter sets / the fixed, seeded point sets of the transverse-Mercator tests
    CONES / cone_sets()           -> the same for the cones
    tm_reference() / cone_reference() -> the exact (x, y) of every point of those sets, computed once per process
    tm_measure(forward, inverse) / cone_measure(forward, inverse) -> an implementation's deviations on those sets; worst(records, key)
"""
import functools

import mpmath as mp
import numpy as np

DPS = 40
WGS84 = dict(a=6378137.0, es=0.0066943799901413165)
_F_AIRY = 1 / 299.32496
_F_INTL = 1 / 297.0


def _wrapped_dlon(lon, lon_0):
    """lon - lon_0 [deg, exact] wrapped to (-180, 180], in radians"""
    d = mp.mpf(float(lon)) - mp.mpf(float(lon_0))
    while d > 180:
        d -= 360
    while d <= -180:
        d += 360
    return mp.radians(d)


# ---- transverse Mercator -----------------------------------------------------------------------------------------------------------
def _psi(p, e):
    return mp.asinh(mp.tan(p)) - e * mp.atanh(e * mp.sin(p))


def _meridian(P, a, es):
    if es == 0:
        return a * P
    return a * (1 - es) * mp.quadgl(lambda t: (1 - es * mp.sin(t) ** 2) ** mp.mpf(-1.5), [0, P])        # (Gauss-Legendre: analytic along the path)


def tm_exact(lat, lon, lat_0=0.0, lon_0=0.0, k_0=0.9996, x_0=500000.0, y_0=0.0, a=6378137.0, es=0.0066943799901413165):
    """(x, y) of one geodetic point [deg, taken as the exact doubles] in a transverse-Mercator CRS, to ~35 digits"""
    with mp.workdps(DPS):
        a, es, k_0 = mp.mpf(float(a)), mp.mpf(float(es)), mp.mpf(float(k_0))
        e = mp.sqrt(es)
        m0 = _meridian(mp.radians(mp.mpf(float(lat_0))), a, es)
        if abs(float(lat)) == 90.0:
            return mp.mpf(float(x_0)), mp.mpf(float(y_0)) + k_0 * (mp.sign(lat) * _meridian(mp.pi / 2, a, es) - m0)
        w = mp.mpc(_psi(mp.radians(mp.mpf(float(lat))), e), _wrapped_dlon(lon, lon_0))
        P = mp.asin(mp.tanh(w))
        for _ in range(60):                                    # Newton, d psi / dP = (1 - e^2) / ((1 - e^2 sin^2 P) cos P): 5 - 6 steps
            d = (_psi(P, e) - w) * (1 - es * mp.sin(P) ** 2) * mp.cos(P) / (1 - es)
            P -= d
            if abs(d) < mp.mpf(10) ** (4 - DPS):
                break
        else:
            raise ArithmeticError(f'no complex latitude for ({lat}, {lon})')
        z = k_0 * (_meridian(P, a, es) - m0)
        return mp.mpf(float(x_0)) + mp.im(z), mp.mpf(float(y_0)) + mp.re(z)


# ---- the cones ---------------------------------------------------------------------------------------------------------------------
def _tsfn(phi, e):
    s = mp.sin(phi)
    return mp.tan((mp.pi / 2 - phi) / 2) / ((1 - e * s) / (1 + e * s)) ** (e / 2)


def _msfn(phi, es):
    return mp.cos(phi) / mp.sqrt(1 - es * mp.sin(phi) ** 2)


def _cone_constant(lat_1, lat_2, es):
    """n of a Lambert cone, Snyder 15-8 (sin lat_1 for a tangent cone), as mpf; call under workdps"""
    es = mp.mpf(float(es)); e = mp.sqrt(es)
    p1, p2 = mp.radians(mp.mpf(float(lat_1))), mp.radians(mp.mpf(float(lat_2)))
    return mp.log(_msfn(p1, es) / _msfn(p2, es)) / mp.log(_tsfn(p1, e) / _tsfn(p2, e)) if abs(p1 - p2) > mp.mpf('1e-10') else mp.sin(p1)


def lcc_exact(lat, lon, lat_1, lat_2, lat_0, lon_0, a, es, x_0=0.0, y_0=0.0):
    """Lambert conformal conic, Snyder 15-1 .. 15-4 (14-1 .. 14-4 on the sphere); a southern cone has n, F and rho negative"""
    with mp.workdps(DPS):
        n = _cone_constant(lat_1, lat_2, es)
        a, es = mp.mpf(float(a)), mp.mpf(float(es)); e = mp.sqrt(es)
        p1, p0 = mp.radians(mp.mpf(float(lat_1))), mp.radians(mp.mpf(float(lat_0)))
        Fc = _msfn(p1, es) * _tsfn(p1, e) ** (-n) / n
        rho0 = a * Fc * _tsfn(p0, e) ** n
        rho = a * Fc * _tsfn(mp.radians(mp.mpf(float(lat))), e) ** n
        th = n * _wrapped_dlon(lon, lon_0)
        return mp.mpf(float(x_0)) + rho * mp.sin(th), mp.mpf(float(y_0)) + rho0 - rho * mp.cos(th)


def stere_exact(lat, lon, lat_0=90.0, lat_ts=None, k_0=1.0, lon_0=0.0, x_0=0.0, y_0=0.0, a=6371229.0, es=0.0):
    """POLAR stereographic (lat_0 = +-90), Snyder 21-33 / 21-34 with 21-39 (true scale at lat_ts) or 21-33 (scale k_0 at the pole,
    lat_ts None); the southern aspect is the northern one of the mirrored latitude with y reversed"""
    if abs(abs(lat_0) - 90.0) > 1e-9:
        raise NotImplementedError('only the polar aspect')
    with mp.workdps(DPS):
        a, es = mp.mpf(float(a)), mp.mpf(float(es)); e = mp.sqrt(es)
        sg = -1 if lat_0 < 0 else 1
        t = _tsfn(sg * mp.radians(mp.mpf(float(lat))), e)
        if lat_ts is not None and abs(abs(lat_ts) - 90.0) > 1e-9:
            pc = abs(mp.radians(mp.mpf(float(lat_ts))))
            rho = a * _msfn(pc, es) * t / _tsfn(pc, e)
        else:
            rho = 2 * a * mp.mpf(float(k_0)) * t / mp.sqrt((1 + e) ** (1 + e) * (1 - e) ** (1 - e))
        dl = _wrapped_dlon(lon, lon_0)
        return mp.mpf(float(x_0)) + rho * mp.sin(dl), mp.mpf(float(y_0)) - sg * rho * mp.cos(dl)


def cone_exact(lat, lon, params):
    kw = dict(params)
    return stere_exact(lat, lon, **kw) if kw.pop('proj', 'lcc') == 'stere' else lcc_exact(lat, lon, **kw)


def deviation(x, y, exact):
    """max(|x - ex|, |y - ey|) [m] per point: doubles against a list of exact (ex, ey)"""
    x = np.asarray(x, dtype=np.float64).ravel(); y = np.asarray(y, dtype=np.float64).ravel()
    with mp.workdps(DPS):
        return np.array([max(abs(float(mp.mpf(float(x[k])) - ex)), abs(float(mp.mpf(float(y[k])) - ey))) if np.isfinite(x[k]) and np.isfinite(y[k])
                         else np.inf for k, (ex, ey) in enumerate(exact)])


def millimetres(exact):
    """the exact (x, y) rounded to the millimetre, as doubles: the inputs of the inverse tests -> (x [n], y [n])"""
    with mp.workdps(DPS):
        return (np.array([float(mp.nint(ex * 1000)) / 1000.0 for ex, _ in exact]), np.array([float(mp.nint(ey * 1000)) / 1000.0 for _, ey in exact]))


# ---- point sets of the transverse-Mercator tests -----------------------------------------------------------------------------------
TM = {
    'utm11n': dict(WGS84, lat_0=0.0, lon_0=-117.0, k_0=0.9996, x_0=500000.0, y_0=0.0),
    'utm35s': dict(WGS84, lat_0=0.0, lon_0=27.0, k_0=0.9996, x_0=500000.0, y_0=10000000.0),
    'utm60n': dict(WGS84, lat_0=0.0, lon_0=177.0, k_0=0.9996, x_0=500000.0, y_0=0.0),
    'osgb': dict(a=6377563.396, es=2 * _F_AIRY - _F_AIRY * _F_AIRY, lat_0=49.0, lon_0=-2.0, k_0=0.9996012717, x_0=400000.0, y_0=-100000.0),
    'snyder': dict(a=6378206.4, es=0.00676866, lat_0=0.0, lon_0=-75.0, k_0=0.9996, x_0=0.0, y_0=0.0),              # Clarke 1866, PP 1395 p. 269
    'sphere': dict(a=6371229.0, es=0.0, lat_0=-30.0, lon_0=170.0, k_0=1.0, x_0=0.0, y_0=0.0),
}
EDGE_LATS = (0.0, 1e-7, -1e-7, 84.0, -84.0, 89.999999, -89.999999)
EDGE_DLON = (0.0, 3.0, -3.0, 35.0, -35.0)
OUT_LATS = (-70.0, -35.0, 0.5, 40.0, 80.0)


def _lon(v):
    """longitudes as a user writes them: in [-180, 180)"""
    return (np.asarray(v, dtype=np.float64) + 180.0) % 360.0 - 180.0


def _frozen(sets):
    """the sets as a tuple with read-only arrays: they are made once and shared by every test of the process"""
    for s in sets:
        for v in s:
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return tuple(sets)


@functools.lru_cache(maxsize=None)
def tm_sets():
    """[(group, name, params, lat [n], lon [n])], group in 'in' | 'pole' | 'anti' | 'out45' | 'out60'.  Seeded: the same doubles in every
    process.  'in': within 35 deg of the central meridian, every latitude short of the pole; 'anti': the wrap of lon - lon_0 (within 35 deg
    of the meridian as well); 'out45' / 'out60': beyond the range the series is good for."""
    rng = np.random.default_rng(20240611)
    sets = []
    for name, p in TM.items():
        la = rng.uniform(-89.5, 89.5, 30); lo = p['lon_0'] + rng.uniform(-35.0, 35.0, 30)
        ela = np.repeat(EDGE_LATS, len(EDGE_DLON)); elo = p['lon_0'] + np.tile(EDGE_DLON, len(EDGE_LATS))
        sets.append(('in', name, p, np.concatenate([la, ela]), _lon(np.concatenate([lo, elo]))))
        sets.append(('pole', name, p, np.array([90.0, 90.0, 90.0, -90.0, -90.0, -90.0]), _lon(p['lon_0'] + np.array([0.0, 20.0, -100.0, 0.0, -20.0, 100.0]))))
        if name not in ('utm35s', 'utm60n'):                  # (relative to the meridian the UTM zones are one case: utm11n stands for them)
            sets.append(('out45', name, p, np.array(OUT_LATS), _lon(p['lon_0'] + 45.0 * np.array([1, -1, 1, -1, 1]))))
            sets.append(('out60', name, p, np.array(OUT_LATS), _lon(p['lon_0'] + 60.0 * np.array([-1, 1, -1, 1, -1]))))
    for name in ('utm60n', 'sphere'):
        p = TM[name]
        sets.append(('anti', name, p, np.array([47.0, -12.5, 71.25]), np.array([-179.0, 181.0, 179.5])))
        # lon_0 as a model header writes it, 0 .. 360: lon - lon_0 is -360 deg before the wrap
        sets.append(('anti', name + '/262.5', dict(p, lon_0=262.5), np.array([38.5, -66.0]), np.array([-97.5, -97.5])))
    return _frozen(sets)


@functools.lru_cache(maxsize=None)
def tm_reference():
    """the exact (x, y) of every set of tm_sets(), in that order: [[(ex, ey)] * n]"""
    return [[tm_exact(float(a), float(b), **p) for a, b in zip(la, lo)] for _, _, p, la, lo in tm_sets()]


# ---- point sets of the cone tests --------------------------------------------------------------------------------------------------
CONES = {
    'hrrr': dict(proj='lcc', lat_1=38.5, lat_2=38.5, lat_0=38.5, lon_0=-97.5, a=6371229.0, es=0.0),
    'snyder': dict(proj='lcc', lat_1=33.0, lat_2=45.0, lat_0=23.0, lon_0=-96.0, a=6378206.4, es=0.00676866),
    'south': dict(WGS84, proj='lcc', lat_1=-30.0, lat_2=-60.0, lat_0=-45.0, lon_0=135.0, x_0=1200000.0, y_0=-350000.0),
    'hrrr-ak': dict(proj='stere', lat_0=90.0, lat_ts=60.0, lon_0=225.0, a=6371229.0, es=0.0),
    'epsg3413': dict(WGS84, proj='stere', lat_0=90.0, lat_ts=70.0, lon_0=-45.0),
    'south71': dict(proj='stere', lat_0=-90.0, lat_ts=-71.0, lon_0=-100.0, a=6378388.0, es=2 * _F_INTL - _F_INTL * _F_INTL),   # Snyder p. 315
    'k0.994': dict(WGS84, proj='stere', lat_0=90.0, lat_ts=None, k_0=0.994, lon_0=0.0, x_0=2000000.0, y_0=2000000.0),          # UPS north
}


@functools.lru_cache(maxsize=None)
def cone_sets():
    """[(name, params, lat [20], lon [20], near_pole [20] bool)]: 16 seeded points over the latitudes the projection is used at and within
    60 deg (LCC) / at every longitude (stereographic), 2 within 1e-6 deg of the projection's pole, 2 within 0.1 deg of the cut meridian"""
    rng = np.random.default_rng(20240612)
    sets = []
    for name, p in CONES.items():
        south = p['lat_0'] < 0
        if p['proj'] == 'lcc':
            la = rng.uniform(20.0, 60.0, 16); lo = p['lon_0'] + rng.uniform(-60.0, 60.0, 16)
        else:
            la = rng.uniform(45.0, 89.5, 16); lo = rng.uniform(-180.0, 180.0, 16)
        la = np.concatenate([la, [90.0 - 9e-7, 90.0 - 3e-7], [40.0, 55.0]])
        lo = np.concatenate([lo, p['lon_0'] + np.array([25.0, -140.0]), p['lon_0'] + 180.0 + np.array([0.05, -0.08])])
        near = np.zeros(20, dtype=bool); near[16:18] = True
        sets.append((name, p, -la if south else la, _lon(lo), near))
    return _frozen(sets)


@functools.lru_cache(maxsize=None)
def cone_reference():
    return [[cone_exact(float(a), float(b), p) for a, b in zip(la, lo)] for _, p, la, lo, _ in cone_sets()]


# ---- the measurement both tests make -----------------------------------------------------------------------------------------------
def tm_measure(forward, inverse):
    """An implementation - forward(lat, lon, params) -> (x, y), inverse(x, y, params) -> (lat, lon), arrays of doubles - against the exact
    mapping, per set of tm_sets(): [dict(group, name, fwd [n], inv [n], x, y, lat, lon)].  fwd: deviation of forward's (x, y) from the exact
    ones [m].  inv: the exact (x, y) rounded to the millimetre go through inverse, its (lat, lon) through the EXACT forward: the distance
    to the input [m] - except in the group 'pole', where inverse gets what forward returned and inv is | |lat| - 90 | [deg] (the longitude
    is free there).  x, y / lat, lon: what forward / inverse returned."""
    out = []
    for (group, name, p, la, lo), ex in zip(tm_sets(), tm_reference()):
        x, y = (np.asarray(v, dtype=np.float64) for v in forward(la, lo, p))
        if group == 'pole':
            la2, lo2 = (np.asarray(v, dtype=np.float64) for v in inverse(x, y, p))
            inv = np.abs(np.abs(la2) - 90.0)
        else:
            X, Y = millimetres(ex)
            la2, lo2 = (np.asarray(v, dtype=np.float64) for v in inverse(X, Y, p))
            ok = np.isfinite(la2) & np.isfinite(lo2)
            back = [tm_exact(float(a), float(b), **p) if f else (mp.inf, mp.inf) for a, b, f in zip(la2, lo2, ok)]
            inv = np.where(ok, deviation(X, Y, back), np.inf)
        out.append(dict(group=group, name=name, fwd=deviation(x, y, ex), inv=inv, x=x, y=y, lat=la2, lon=lo2))
    return out


def cone_measure(forward, inverse):
    """The same for the cones, per set of cone_sets(): [dict(name, near, fwd [20], inv [20], lat, lon)]; forward(lat, lon, params) ->
    (x, y), inverse(x, y, params) -> (lat, lon) with params a dict of CONES."""
    out = []
    for (name, p, la, lo, near), ex in zip(cone_sets(), cone_reference()):
        x, y = forward(la, lo, p)
        X, Y = millimetres(ex)
        la2, lo2 = (np.asarray(v, dtype=np.float64) for v in inverse(X, Y, p))
        ok = np.isfinite(la2) & np.isfinite(lo2)
        back = [cone_exact(float(a), float(b), p) if f else (mp.inf, mp.inf) for a, b, f in zip(la2, lo2, ok)]
        out.append(dict(name=name, near=near, fwd=deviation(x, y, ex), inv=np.where(ok, deviation(X, Y, back), np.inf), lat=la2, lon=lo2))
    return out


def worst(records, key, **where):
    """the largest records[.][key] over the records that match `where` (e.g. group='in')"""
    return max(float(np.max(r[key])) for r in records if all(r[k] == v for k, v in where.items()))


def lcc_pole_quantum(k):
    """[20] m: how far ONE ulp of a latitude next to +-90 deg (1.42e-14 deg) moves a point of cone_sets()[k], a Lambert cone: d rho =
    |n| rho d(colat) / colat, with rho the exact distance from the cone's apex (x_0, y_0 + rho0).  At a colatitude of 1e-6 deg that is
    1.4e-8 of rho, tens of metres there (rho ~ colat^n, n ~ 0.6): no inverse that returns degrees as doubles can close better."""
    name, p, la, lo, near = cone_sets()[k]
    with mp.workdps(DPS):
        ax, ay = cone_exact(90.0 if p['lat_0'] > 0 else -90.0, p['lon_0'], p)            # the apex: rho = 0 there
        rho = np.array([float(mp.hypot(ex - ax, ey - ay)) for ex, ey in cone_reference()[k]])
        n = abs(float(_cone_constant(p['lat_1'], p['lat_2'], p['es'])))
    return n * rho * np.spacing(90.0 - 1e-6) / (90.0 - np.abs(la))
