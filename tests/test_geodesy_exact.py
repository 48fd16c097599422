"""The oracle's geodesy against the EXACT mathematics of the ellipsoid, evaluated with 40 significant digits (mpmath).

The reference delegates WGS 84 <-> ECEF and the model projections to pyproj / PROJ, which is absent from the image: the oracle
restates PROJ's published formulas and is pinned on worked examples that carry millimetres (IOGP GN 7-2, Snyder).  This file
adds what those examples cannot: the defining equations themselves, solved to 40 digits, over the whole range the delay path
uses (heights -500 m ... 85 km, every latitude).  Findings it asserts:

  * geodetic -> ECEF and the conic projections: the restatements are exact to rounding (< 5e-9 m / 2e-8 m);
  * transverse Mercator: Krueger's series to n^6 is exact to rounding (< 1e-8 m) within 35 degrees of the central meridian, poles
    included; its truncation is 2e-8 m at 45 degrees and 1.2e-5 m at 60 degrees (the exact mapping: tests/projection_exact.py);
  * ECEF -> geodetic: PROJ's published inverse is ONE Bowring step, whose truncation grows with height squared - 1e-8 m at 1 km,
    1e-6 m at 10 km, 1.6e-5 m at 40 km, 7e-5 m at 85 km in height (6e-10 degrees in latitude).  The restatement reproduces
    that formula (it is the parity target: the reference calls PROJ); this test bounds how far formula and exact ellipsoid are
    apart, so that ANY PROJ version within that envelope gives the same delays: integrated against the refractivity gradient
    (270e-6/8 km, scale height 8 km) an error of 7e-5 (h / 85 km)^2 m moves a zenith delay by 3e-10 m, a slant one by < 1e-9 m."""
import numpy as np
import pytest

from oracle import raider_oracle as O

mp = pytest.importorskip('mpmath')

from tests import projection_exact as P                   # noqa: E402  (needs mpmath)

A = mp.mpf(6378137)
F = 1 / mp.mpf('298.257223563')
ES = 2 * F - F * F


def _exact_lla2ecef(lat, lon, h):
    phi, lam = mp.radians(mp.mpf(lat)), mp.radians(mp.mpf(lon))
    N = A / mp.sqrt(1 - ES * mp.sin(phi) ** 2)
    return (N + h) * mp.cos(phi) * mp.cos(lam), (N + h) * mp.cos(phi) * mp.sin(lam), (N * (1 - ES) + h) * mp.sin(phi)


def _exact_ecef2lla(x, y, z):
    """Geodetic latitude / height of an ECEF point: Newton on the latitude equation p tan(phi) - z = e^2 N(phi) sin(phi)."""
    x, y, z = mp.mpf(x), mp.mpf(y), mp.mpf(z)
    p = mp.sqrt(x * x + y * y)
    f = lambda phi: p * mp.sin(phi) - z * mp.cos(phi) - ES * A * mp.sin(phi) * mp.cos(phi) / mp.sqrt(1 - ES * mp.sin(phi) ** 2)
    phi = mp.findroot(f, mp.atan2(z, p * (1 - ES)))
    N = A / mp.sqrt(1 - ES * mp.sin(phi) ** 2)
    h = p * mp.cos(phi) + z * mp.sin(phi) - A * A / N                     # = p/cos(phi) - N, stable at the poles
    return mp.degrees(mp.atan2(y, x)), mp.degrees(phi), h


def test_geodetic_ecef_conversions_against_40_digit_arithmetic():
    mp.mp.dps = 40
    rng = np.random.default_rng(0)
    lat = np.concatenate([rng.uniform(-90, 90, 60), [0.0, 89.999, -89.999, 45.0, 1e-9]])
    lon = np.concatenate([rng.uniform(-180, 180, 60), [0.0, 179.999, -179.999, 90.0, -90.0]])
    h = np.concatenate([rng.uniform(-500, 85000, 60), [0.0, 85000.0, -500.0, 41000.0, 10.0]])
    x, y, z = O.lla2ecef(lat, lon, h)
    lo2, la2, h2 = O.ecef2lla(x, y, z)
    worst_fwd = worst_ang = 0.0
    worst_h = {1000.0: 0.0, 10000.0: 0.0, 40000.0: 0.0, 85000.0: 0.0}
    for k in range(lat.size):
        ex = _exact_lla2ecef(float(lat[k]), float(lon[k]), float(h[k]))
        worst_fwd = max(worst_fwd, *(abs(float(mp.mpf(float(v)) - e)) for v, e in zip((x[k], y[k], z[k]), ex)))
        elon, elat, eh = _exact_ecef2lla(float(x[k]), float(y[k]), float(z[k]))      # exact inverse OF THE DOUBLES the oracle was given
        dh = abs(float(mp.mpf(float(h2[k])) - eh))
        for top in worst_h:
            if h[k] <= top:
                worst_h[top] = max(worst_h[top], dh)
        worst_ang = max(worst_ang, abs(float(mp.mpf(float(la2[k])) - elat)), abs(float(((mp.mpf(float(lo2[k])) - elon + 180) % 360) - 180)))
    assert worst_fwd < 5e-9, worst_fwd                                     # forward: pure rounding (a few ulp of 6.4e6 m)
    # inverse: the one-step Bowring formula's truncation envelope (grows ~h^2); rounding alone is ~3e-9 m
    assert worst_h[1000.0] < 3e-8 and worst_h[10000.0] < 2e-6 and worst_h[40000.0] < 3e-5 and worst_h[85000.0] < 1e-4, worst_h
    assert worst_ang < 1e-9, worst_ang                                     # degrees: 1e-9 deg = 1e-4 m on the ground, at 85 km


def test_conic_projections_against_40_digit_arithmetic():
    """lcc_forward / stere_forward and their inverses: Snyder's closed forms evaluated in 40 digits (the formulas ARE the definition
    of the projection; PROJ implements the same ones) - bounds the double-precision rounding of the restatement, metres at 1e-8."""
    mp.mp.dps = 40
    lcc, stere = P.lcc_exact, P.stere_exact
    rng = np.random.default_rng(1)
    cases = [dict(lat_1=38.5, lat_2=38.5, lat_0=38.5, lon_0=-97.5, a=6371229.0, es=0.0),                       # HRRR
             dict(lat_1=33.0, lat_2=45.0, lat_0=23.0, lon_0=-96.0, a=6378206.4, es=0.00676866)]                # Snyder's ellipsoidal case
    for kw in cases:
        la = rng.uniform(20, 60, 40); lo = rng.uniform(-130, -65, 40)
        x, y = O.lcc_forward(la, lo, **kw)
        la2, lo2 = O.lcc_inverse(x, y, **kw)
        for k in range(la.size):
            ex, ey = lcc(float(la[k]), float(lo[k]), **kw)
            assert abs(float(mp.mpf(float(x[k])) - ex)) < 2e-8 and abs(float(mp.mpf(float(y[k])) - ey)) < 2e-8
        assert np.abs(la2 - la).max() < 1e-12 and np.abs(lo2 - lo).max() < 1e-12
    ak = dict(lat_0=90.0, lat_ts=60.0, lon_0=225.0, a=6371229.0, es=0.0)                                         # HRRR-AK
    ell = dict(lat_0=90.0, lat_ts=70.0, lon_0=-45.0, a=6378137.0, es=0.0066943799901413165)                     # EPSG:3413's parameters
    for kw in (ak, ell):
        la = rng.uniform(45, 89.5, 40); lo = rng.uniform(-180, 180, 40)
        x, y = O.stere_forward(la, lo, **kw)
        for k in range(la.size):
            ex, ey = stere(float(la[k]), float(lo[k]), **kw)
            assert abs(float(mp.mpf(float(x[k])) - ex)) < 2e-8 and abs(float(mp.mpf(float(y[k])) - ey)) < 2e-8


def test_transverse_mercator_against_40_digit_arithmetic():
    """tm_forward / tm_inverse (Krueger's series to n^6, twelve typed rational coefficients) against the EXACT mapping - the analytic
    continuation of the meridian distance in the isometric latitude, solved in 40 digits without any series (tests/projection_exact.py) -
    on six parameter sets (three UTM zones, OSGB on Airy with lat_0 = 49, Snyder's Clarke 1866 case, a sphere with lat_0 = -30): 65
    points per set within 35 degrees of the central meridian at latitudes up to +-89.999999, the poles, the antimeridian wrap.  Forward:
    within 1e-8 m (5 ulp of 1e7 m; measured 6.7e-9 m).  Inverse: the exact (x, y) rounded to the millimetre come back, through the exact
    forward, within 1e-8 m (measured 5.2e-9 m).  What a typed coefficient does here: 61/240 -> 61/241 in al[2] gives 8.0e-4 m forward,
    17/480 -> 17/481 in be[2] 5.6e-5 m back (either also breaks the 1e-11 degree closure of tests/test_oracle_golden.py); n^3 / 1000 added
    to BOTH, a slip the two series share, 7.6e-4 m and 7.7e-4 m - and closure and the printed examples stay green.
    Beyond 35 degrees the assertion is the series' own TRUNCATION, measured on this reference, not rounding: 2.1e-8 m at 45 degrees from
    the meridian (bound 1e-7 m), 1.2e-5 m at 60 degrees (bound 1e-4 m); the inverse closes within 4.6e-9 m / 5.4e-7 m there."""
    rec = P.tm_measure(lambda la, lo, p: O.tm_forward(la, lo, **p), lambda x, y, p: O.tm_inverse(x, y, **p))
    for r in rec:
        print(f"{r['group']:6s} {r['name']:14s} forward {r['fwd'].max():.3e} m   inverse {r['inv'].max():.3e} {'deg' if r['group'] == 'pole' else 'm'}")
        assert np.isfinite(r['x']).all() and np.isfinite(r['y']).all() and np.isfinite(r['lat']).all() and np.isfinite(r['lon']).all()
        assert r['lon'].min() >= -180.0 and r['lon'].max() <= 180.0
    for group in ('in', 'anti'):
        assert P.worst(rec, 'fwd', group=group) < 1e-8 and P.worst(rec, 'inv', group=group) < 1e-8, group
    # the poles: x = x_0 and the exact northing k_0 (+-M(pi/2) - M(lat_0)); the inverse of that point is the pole
    assert P.worst(rec, 'fwd', group='pole') < 1e-8 and P.worst(rec, 'inv', group='pole') < 1e-9
    assert P.worst(rec, 'fwd', group='out45') < 1e-7 and P.worst(rec, 'inv', group='out45') < 1e-7
    assert P.worst(rec, 'fwd', group='out60') < 1e-4 and P.worst(rec, 'inv', group='out60') < 1e-4
    assert P.worst(rec, 'fwd', group='out60') > 1e-6            # (what is recorded is the truncation: it must be visible in that group)


def test_cones_near_the_pole_and_the_cut_meridian_against_40_digit_arithmetic():
    """The point sets of the device test (tests/projection_exact.py: cone_sets) on the oracle: HRRR, Snyder's ellipsoidal cone, a
    SOUTHERN cone with false origin, HRRR-AK, EPSG:3413's parameters, a south-polar lat_ts = -71 case and the k_0 = 0.994 variant, 20
    points each with two within 1e-6 degrees of the projection's pole and two within 0.1 degrees of the cut meridian.  Within 2e-8 m,
    forward and (millimetre-rounded (x, y) -> inverse -> exact forward) back, with ONE exception, which is the number format and not the
    formulas: next to the pole of a Lambert cone rho ~ colat^n (n ~ 0.6) is tens of metres at a colatitude of 1e-6 degrees, which a double
    near 90 degrees / pi/2 resolves to 1e-8 of itself only.  Forward (pi/2 - phi is formed in doubles): measured 8e-8 .. 5e-7 m.  Inverse:
    ONE ulp of the returned latitude is 5e-7 .. 1.5e-6 m (projection_exact.lcc_pole_quantum); four are allowed."""
    rec = P.cone_measure(O.project_forward, O.project_inverse)
    for k, r in enumerate(rec):
        near = r['near'] & (P.cone_sets()[k][1]['proj'] == 'lcc')
        print(f"{r['name']:10s} forward {r['fwd'][~near].max():.3e} m   inverse {r['inv'][~near].max():.3e} m   next to an LCC pole: {r['fwd'][near]} {r['inv'][near]}")
        assert r['fwd'][~near].max() < 2e-8 and r['inv'][~near].max() < 2e-8, r['name']
        assert r['lon'].min() >= -180.0 and r['lon'].max() <= 180.0
        if near.any():
            q = P.lcc_pole_quantum(k)[near]
            assert (r['fwd'][near] < 4 * q).all() and (r['inv'][near] < 4 * q).all(), (r['name'], q)


ERFA_PY = '/opt/conda/bin/python3.9'          # an Anaconda interpreter in the image carries pyerfa (the IAU SOFA routines, with astropy)


def test_geodetic_ecef_conversions_against_erfa(tmp_path):
    """A THIRD party's code for the same conversions: ERFA / SOFA `gd2gc` and `gc2gd` (Fukushima's closed-form inverse, no truncation)
    on 200 000 points over the range the delay path uses - the 40-digit test above covers 65.  Forward: rounding only.  Inverse: the
    oracle restates PROJ's ONE Bowring step, so its height departs from ERFA's by that step's truncation (~h^2; same envelope as
    above), its latitude by < 1e-9 degrees."""
    import os
    import subprocess
    if not os.path.exists(ERFA_PY):
        pytest.skip('no interpreter with pyerfa in this image')
    script = (
        "import sys, numpy as np\n"
        "try:\n    import erfa\nexcept Exception:\n    sys.exit(77)\n"
        "d = np.load(sys.argv[1])\n"
        "xyz = erfa.gd2gc(1, np.radians(d['lon']), np.radians(d['lat']), d['h'])\n"          # 1 = WGS84
        "elong, phi, height = erfa.gc2gd(1, d['xyz'])\n"
        "np.savez(sys.argv[2], xyz=xyz, lon=np.degrees(elong), lat=np.degrees(phi), h=height)\n")
    rng = np.random.default_rng(5)
    n = 200000
    lat = rng.uniform(-90, 90, n); lon = rng.uniform(-180, 180, n); h = rng.uniform(-500, 85000, n)
    x, y, z = O.lla2ecef(lat, lon, h)
    np.savez(tmp_path / 'in.npz', lat=lat, lon=lon, h=h, xyz=np.stack([x, y, z], -1))
    r = subprocess.run([ERFA_PY, '-c', script, str(tmp_path / 'in.npz'), str(tmp_path / 'out.npz')], capture_output=True, text=True, timeout=600,
                       env={k: v for k, v in os.environ.items() if not k.startswith('PYTHON')})
    if r.returncode == 77:
        pytest.skip('pyerfa is not importable')
    assert r.returncode == 0, r.stderr[-2000:]
    e = np.load(tmp_path / 'out.npz')
    assert np.abs(np.stack([x, y, z], -1) - e['xyz']).max() < 5e-9                      # forward: a few ulp of 6.4e6 m
    lo2, la2, h2 = O.ecef2lla(x, y, z)
    dh = np.abs(h2 - e['h'])
    for top, bound in ((1000.0, 3e-8), (10000.0, 2e-6), (40000.0, 3e-5), (85000.0, 1e-4)):
        assert dh[h <= top].max() < bound, (top, dh[h <= top].max())
    assert np.abs(la2 - e['lat']).max() < 1e-9
    dlon = np.abs(((lo2 - e['lon'] + 180.0) % 360.0) - 180.0)
    assert dlon[np.abs(lat) < 89.99].max() < 1e-12
    # and ERFA's own inverse returns the inputs: the two authorities (40 digits, SOFA) agree with each other through the oracle's forward
    assert np.abs(e['h'] - h).max() < 2e-8 and np.abs(e['lat'] - lat).max() < 1e-12
