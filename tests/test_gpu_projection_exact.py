"""GPU: tm_kernel and cone_kernel (csrc/proj_kernels.h, csrc/geodesy.h) against the EXACT projections in 40 digits (tests/projection_exact.py),
with the CPU oracle measured on the same points as the second yardstick: the device may be 4 x as far from the exact mapping as the oracle
is (the device math library differs from glibc by an ulp or two per call, across six sin / cosh pairs), or 1e-8 m - 5 ulp of 1e7 m - where
the oracle is closer than a quarter of that.  Never the kernel's own output.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import raider_oracle as O                      # noqa: E402

from tests import projection_exact as P                    # noqa: E402  (imports mpmath: its absence is an error here, not a skip)

FLOOR = 1e-8                                               # m


def _bound(oracle_worst):
    return max(FLOOR, 4.0 * oracle_worst)


def _dev_forward(la, lo, p):
    from raider_amd.utilFcns import transverse_mercator
    y, x = transverse_mercator(la, lo, p)
    return x, y


def _dev_inverse(x, y, p):
    from raider_amd.utilFcns import transverse_mercator
    return transverse_mercator(y, x, p, inverse=True)


def _cone_forward(la, lo, p):
    from raider_amd.utilFcns import conic
    y, x = conic(la, lo, p)
    return x, y


def _cone_inverse(x, y, p):
    from raider_amd.utilFcns import conic
    return conic(y, x, p, inverse=True)


@pytest.fixture(scope='module')
def tm_oracle():
    return P.tm_measure(lambda la, lo, p: O.tm_forward(la, lo, **p), lambda x, y, p: O.tm_inverse(x, y, **p))


@pytest.fixture(scope='module')
def tm_device():
    return P.tm_measure(_dev_forward, _dev_inverse)


def _report(what, dev, ora, bound):
    print(f'{what}: device {dev:.3e}   oracle {ora:.3e}   bound {bound:.3e}')


def test_forward_kernel_within_35_degrees_at_the_poles_and_across_the_antimeridian(tm_oracle, tm_device):
    """transverse_mercator(lat, lon) on the six parameter sets (lat_0 != 0, a sphere, Airy, Clarke 1866, a southern false northing, a zone at
    the antimeridian) against the exact mapping.  Measured on an MI355X, worst over the sets: 6.0e-9 m within 35 degrees (the
    oracle: 6.7e-9 m), 3.6e-9 m at the poles (3.6e-9 m), 2.5e-9 m across the antimeridian (2.5e-9 m)."""
    for group in ('in', 'pole', 'anti'):
        d, o = P.worst(tm_device, 'fwd', group=group), P.worst(tm_oracle, 'fwd', group=group)
        _report(f'forward {group}', d, o, _bound(o))
        assert o < FLOOR                                        # (the yardstick itself: tests/test_geodesy_exact.py)
        assert d <= _bound(o), group
    for r in tm_device:
        assert np.isfinite(r['x']).all() and np.isfinite(r['y']).all(), r['name']


def test_inverse_kernel_closes_through_the_exact_forward(tm_oracle, tm_device):
    """transverse_mercator(y, x, inverse=True) of the exact (x, y) rounded to the millimetre, its (lat, lon) pushed through the exact forward:
    the distance to the input.  At the poles the kernel inverts its own forward result: |lat| = 90 within 1e-9 degrees (the longitude is free).
    Longitudes come out in [-180, 180], everything finite.  Measured on an MI355X, worst over the sets: 5.2e-9 m within 35 degrees (the oracle:
    5.2e-9 m), 2.3e-9 m across the antimeridian (2.3e-9 m); the poles come back as |lat| = 90 exactly."""
    for group in ('in', 'anti'):
        d, o = P.worst(tm_device, 'inv', group=group), P.worst(tm_oracle, 'inv', group=group)
        _report(f'inverse {group}', d, o, _bound(o))
        assert o < FLOOR
        assert d <= _bound(o), group
    d = P.worst(tm_device, 'inv', group='pole')
    print(f'inverse of the pole: | |lat| - 90 | = {d:.3e} deg')
    assert d < 1e-9
    for r in tm_device:
        assert np.isfinite(r['lat']).all() and np.isfinite(r['lon']).all(), r['name']
        assert r['lon'].min() >= -180.0 and r['lon'].max() <= 180.0, r['name']


def _angles(tm_oracle, tm_device, where):
    """worst |lat - oracle's|, |lon - oracle's| [deg] over the in-range and antimeridian points with where(lat of the point)"""
    wl = wo = 0.0
    for d, o, s in zip(tm_device, tm_oracle, P.tm_sets()):
        m = where(s[3])
        if d['group'] in ('in', 'anti') and m.any():
            dl = np.abs(d['lat'] - o['lat'])[m]; do = np.abs((d['lon'] - o['lon'] + 180.0) % 360.0 - 180.0)[m]
            print(f"{d['group']:5s} {d['name']:14s} lat {dl.max():.3e} deg   lon {do.max():.3e} deg (at lat {s[3][m][int(np.argmax(do))]})")
            wl = max(wl, dl.max()); wo = max(wo, do.max())
    return wl, wo


def test_inverse_kernel_returns_the_oracles_angles(tm_oracle, tm_device):
    """The same millimetre-rounded inputs: the device's latitude within 1e-12 degrees of the oracle's at EVERY point, its longitude at
    every point up to +-89.5 degrees - the closure bound of the suite.  Measured on an MI355X: 1.4e-14 degrees and 2.8e-14 degrees.  (The
    twenty points at +-89.999999 degrees are the test below.)"""
    wl, _ = _angles(tm_oracle, tm_device, lambda la: np.abs(la) <= 90.0)
    _, wo = _angles(tm_oracle, tm_device, lambda la: np.abs(la) <= 89.5)
    assert wl < 1e-12 and wo < 1e-12, (wl, wo)


def test_inverse_kernel_returns_the_oracles_longitude_next_to_the_pole(tm_oracle, tm_device):
    """The bound above on the longitude at latitude +-89.999999 degrees as well, where it pins the rounding of tm_setup itself: xi =
    (y - y_0) / kA + xi0 is pi/2 - 1.7e-8 there, rounded to 2.2e-16, and the longitude is atan2(sinh eta', cos xi'), so ONE ulp of xi, hence
    of kA, is 1.3e-8 of the longitude - 4e-7 degrees, 1e-9 m on the ground.  kA = k_0 a / (1 + n) (...) multiplied out from the left, in
    tm_setup and in the oracle alike; k_0 (a / (1 + n) (...)) is one ulp away on WGS 84 and Airy.  Measured on an MI355X: 2.8e-14 degrees."""
    _, wo = _angles(tm_oracle, tm_device, lambda la: np.abs(la) > 89.5)
    assert wo < 1e-12, wo


def test_beyond_35_degrees_the_device_stays_inside_the_series_truncation(tm_oracle, tm_device):
    """45 and 60 degrees from the central meridian: what is asserted is the envelope of the n^6 series' truncation recorded on the oracle
    (tests/test_geodesy_exact.py: 2.1e-8 m and 1.2e-5 m, bounds 1e-7 m and 1e-4 m), not rounding."""
    for group, bound in (('out45', 1e-7), ('out60', 1e-4)):
        for key in ('fwd', 'inv'):
            d, o = P.worst(tm_device, key, group=group), P.worst(tm_oracle, key, group=group)
            _report(f'{key} {group}', d, o, bound)
            assert o < bound and d < bound, (group, key)


def _pool(p):
    """the 390 in-range points of all six sets, moved to the central meridian of `p`"""
    ins = [s for s in P.tm_sets() if s[0] == 'in']
    la = np.concatenate([s[3] for s in ins])
    lo = np.concatenate([(s[4] - s[2]['lon_0'] + 180.0) % 360.0 - 180.0 + p['lon_0'] for s in ins])
    return la, lo


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def test_launch_edges_and_the_second_trip_of_the_grid_stride_loop():
    """n = 1, 63, 64, 65, 255, 257: the bits of the matching slice of the full call.  n = 256 * 8 * num_cus + 3: the launch is capped at
    8 * num_cus blocks, so three threads make a second trip; every repeat of the tiled set has the bits of the first.  Both directions."""
    from raider_amd._lib import Context
    p = P.TM['osgb']
    la, lo = _pool(p)
    x, y = _dev_forward(la, lo, p)
    la2, lo2 = _dev_inverse(x, y, p)
    for n in (1, 63, 64, 65, 255, 257):
        xn, yn = _dev_forward(la[:n], lo[:n], p)
        assert _same(xn, x[:n]) and _same(yn, y[:n]), n
        an, bn = _dev_inverse(x[:n], y[:n], p)
        assert _same(an, la2[:n]) and _same(bn, lo2[:n]), n
    cus = Context.default().device_info()[1]
    assert cus > 0
    n = 256 * 8 * cus + 3
    xb, yb = _dev_forward(np.resize(la, n), np.resize(lo, n), p)
    assert xb.shape == (n,) and _same(xb, np.resize(x, n)) and _same(yb, np.resize(y, n))
    ab, bb = _dev_inverse(np.resize(x, n), np.resize(y, n), p)
    assert _same(ab, np.resize(la2, n)) and _same(bb, np.resize(lo2, n))


def test_a_non_finite_input_is_nan_in_its_own_slot_only():
    p = P.TM['utm35s']
    la, lo = _pool(p)
    la, lo = la[:70], lo[:70]
    x, y = _dev_forward(la, lo, p)
    la2, lo2 = _dev_inverse(x, y, p)
    bad = np.zeros(72, dtype=bool); bad[[20, 41]] = True
    for v in (np.inf, -np.inf):
        lb = np.empty(72); lb[~bad] = la; lb[20] = np.nan; lb[41] = v
        ob = np.empty(72); ob[~bad] = lo; ob[bad] = 27.5
        xb, yb = _dev_forward(lb, ob, p)
        assert np.isnan(xb[bad]).all() and np.isnan(yb[bad]).all()
        assert _same(xb[~bad], x) and _same(yb[~bad], y)
        yv = np.empty(72); yv[~bad] = y; yv[20] = np.nan; yv[41] = v
        xv = np.empty(72); xv[~bad] = x; xv[bad] = 512345.0
        ab, bb = _dev_inverse(xv, yv, p)
        assert np.isnan(ab[bad]).all() and np.isnan(bb[bad]).all()
        assert _same(ab[~bad], la2) and _same(bb[~bad], lo2)


def test_grid_route_is_the_inverse_kernel_on_the_meshgrid():
    """grid_geodetic on a 5 x 4 OSGB grid and on one 30 degrees east of the meridian of UTM 11N, NumPy and device tensors: the bits of the
    inverse kernel on the meshgrid, hence within the inverse bound of the exact mapping."""
    import raider_amd as R
    import torch
    from raider_amd._lib import RDR_GRID_TM
    from raider_amd.utilFcns import tm_abi
    cx, cy = O.tm_forward(40.0, -87.0, **P.TM['utm11n'])
    grids = ((P.TM['osgb'], 100000.0 + 130000.0 * np.arange(5), 1100000.0 - 300000.0 * np.arange(4)),
             (P.TM['utm11n'], np.round(cx) + 20000.0 * (np.arange(5) - 2), np.round(cy) - 20000.0 * (np.arange(4) - 1.5)))
    for p, xg, yg in grids:
        xx, yy = np.meshgrid(xg, yg)
        la, lo = _dev_inverse(xx, yy, p)
        crs = (RDR_GRID_TM, tm_abi(p))
        gla, glo = R.grid_geodetic(crs, xg, yg, device=None)
        assert gla.shape == (4, 5) and _same(gla, la) and _same(glo, lo)
        tla, tlo = R.grid_geodetic(crs, torch.from_numpy(xg).cuda(), torch.from_numpy(yg).cuda())
        torch.cuda.synchronize()
        assert tla.is_cuda and _same(tla.cpu().numpy(), la) and _same(tlo.cpu().numpy(), lo)
        ola, olo = O.tm_inverse(xx, yy, **p)
        res = lambda a, b: P.deviation(xx, yy, [P.tm_exact(float(u), float(v), **p) for u, v in zip(np.ravel(a), np.ravel(b))]).max()
        d, o = res(gla, glo), res(ola, olo)
        _report('grid nodes through the exact forward', d, o, _bound(o))
        assert o < FLOOR and d <= _bound(o)


def test_a_continental_station_network_in_one_utm_zone():
    """variogram.utm_common_center: 40 stations over CONUS land in the zone of their median (14 north), up to 32 degrees from its meridian"""
    from raider_amd.utilFcns import utm_params
    from raider_amd.variogram import utm_common_center, utm_zone
    rng = np.random.default_rng(5)
    lon = rng.uniform(-125.0, -67.0, 40); lat = rng.uniform(25.0, 49.0, 40)
    assert utm_zone(np.median(lon), np.median(lat)) == (14, True)
    p = utm_params(32614)
    assert p['lon_0'] == -99.0 and np.abs(lon - p['lon_0']).max() > 25.0
    x, y = utm_common_center(lon, lat)
    exact = [P.tm_exact(float(a), float(b), **p) for a, b in zip(lat, lon)]
    ox, oy = O.tm_forward(lat, lon, **p)
    d, o = P.deviation(x, y, exact).max(), P.deviation(ox, oy, exact).max()
    _report('stations', d, o, _bound(o))
    assert o < FLOOR and d <= _bound(o)


def test_cone_kernel_against_the_closed_forms():
    """utilFcns.conic, forward and (millimetre-rounded exact (x, y) -> inverse -> exact forward) back, on HRRR, Snyder's ellipsoidal cone, a
    southern cone with a false origin, HRRR-AK, EPSG:3413's parameters, a south-polar lat_ts = -71 case and the k_0 = 0.994 variant; 20 points
    each, two within 1e-6 degrees of the projection's pole, two within 0.1 degrees of the cut meridian.  The rule of the transverse-Mercator
    tests, per set.  The oracle is within 2e-8 m of the closed forms on these points EXCEPT next to the pole of a Lambert cone, where the
    double next to 90 degrees / pi/2 resolves the colatitude to 1e-8 of itself only and rho ~ colat^n is tens of metres (tests/
    test_geodesy_exact.py, which bounds the oracle there by the ulp of the latitude, projection_exact.lcc_pole_quantum).  A point next to a
    Lambert pole where the oracle is NOT within 2e-8 m leaves the set's rule, forward or back, and gets a bound of its own: 4 x the oracle's
    error on that same point (both sides form pi/2 - phi, and phi from t, with the same IEEE operations).  Every other point, next to a
    pole or not, stays under the rule of its set.  Measured on an MI355X, worst over the points under the set's rule: forward 8.0e-9 m (the
    oracle: 9.9e-9 m), inverse 1.09e-8 m (1.09e-8 m), both on the southern cone; at the loosened points the device has the oracle's
    error to 7 digits, 8e-8 .. 3.4e-7 m forward, 2.8e-8 .. 9.3e-7 m back."""
    ora = P.cone_measure(O.project_forward, O.project_inverse)
    dev = P.cone_measure(_cone_forward, _cone_inverse)
    for k, (d, o) in enumerate(zip(dev, ora)):
        near = d['near'] & (P.cone_sets()[k][1]['proj'] == 'lcc')
        for key in ('fwd', 'inv'):
            loose = near & (o[key] >= 2e-8)
            dw, ow = d[key][~loose].max(), o[key][~loose].max()
            _report(f"{d['name']} {key}", dw, ow, _bound(ow))
            assert ow < 2e-8 and dw <= _bound(ow), (d['name'], key)
            if loose.any():
                print(f"{d['name']} {key} next to the pole: device {d[key][loose]}   oracle {o[key][loose]}   one ulp of latitude {P.lcc_pole_quantum(k)[loose]}")
                assert (d[key][loose] <= 4.0 * o[key][loose]).all(), (d['name'], key)
        assert np.isfinite(d['lat']).all() and d['lon'].min() >= -180.0 and d['lon'].max() <= 180.0
