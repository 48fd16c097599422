"""The documented accuracy of the light ray geometry, asserted (CPU; DESIGN.md B.3 "Ray polynomials").

tests/ray_poly_model.py restates the design of the light path in extended precision.  Here that model is compared with the reference's
geodesy (raider_oracle.ecef2lla, lcc_forward, build_ray) and with a converged height over the region the static classification
admits: the rays tools/ray_poly_probe.py draws (seed 0) plus rays placed within 2 % of each clause's limit, where the maxima lie.
Every figure the kernels' comments and DESIGN.md quote for the design is a constant of this module.  A figure followed by
`# measured` did not hold as documented before this module existed: it is the worst case of this sweep (seed 0) x 1.5, a margin for
a finite sample of a smooth maximum, and DESIGN.md B.3 carries the measured value."""
import re
from pathlib import Path

import numpy as np
import pytest

from oracle import raider_oracle as O
from tests import ray_poly_model as M
from tests.test_gpu_ray_instantiations import LCC

LD = M.LD
SEED = 0
N_RANDOM, N_EDGE = 6000, 160                   # per clause (4 clauses: at least 500 admitted edge rays, asserted)
NPTS = 401
CSRC = Path(__file__).resolve().parent.parent / 'raider_amd' / 'csrc'

# DESIGN.md B.3, metres: (every admitted ray, rays shorter than 100 km)
# (the lat / lon figures were documented for a longitude-travel limit of 0.2 rad, where rays on the limit reach 6.3e-4 m and 1.8e-3 m;
# with the limit at 0.12 rad this sweep measures 5.9e-5 / 3.1e-5 m (lat) and 1.5e-4 / 9.4e-5 m (lon))
BOUND_H = (1.5 * 2.52e-7, 5e-9)                # measured (documented: 2.5e-7, which the cone's sweep passes by 0.7 %) | as documented
BOUND_LAT = (3.5e-4, 1.4e-4)
BOUND_LON = (1.2e-3, 4.8e-4)
# metres of height between the model's crossings and the reference's, by model top: as documented to 40 km; at 80 km measured
BOUND_CROSSING = {15000.0: 2e-5, 40000.0: 2e-5, 80000.0: 1.5 * 6.61e-5}
BOUND_XPOLY = ((60.0, 1e-10), (70.0, 7e-9), (85.0, 3e-6))   # crossing polynomial against the plain three-step iteration, 80 km top
BOUND_ASIN = 1.4e-11                           # rad (geodesy_fast.h: asin_small)
BOUND_LCC_SERIES = (9e-15, 3e-17, 1e-19)       # next-term sizes, relative: atanh, exp, sin / cos (geodesy_fast.h: ecef2lcc_sphere)


# ---- the sweep ------------------------------------------------------------------------------------------------------------------------


def _probe_rays(n, rng):
    """lat, lon, inc, hd, zref, ht as tools/ray_poly_probe.py draws them, call by call"""
    rows = []
    for _ in range(n):
        lat0 = rng.uniform(-89.5, 89.5); inc = rng.uniform(0, 86); hd = rng.uniform(-180, 180)
        zref = rng.choice([15000., 40000., 80000.]); ht = rng.choice([0., -100., 3000.]); lon0 = rng.uniform(-170, 170)
        rows.append((lat0, lon0, inc, hd, zref, ht))
    return np.array(rows).T


def _edge_rays(n, rng, lcc=False):
    """rays within 2 % of each clause's limit (on the admitted side): gam -> 0.035, gam -> 0.12 (c0 - gam), c0 -> gam + 0.02 and, on a
    cone, gam -> 0.09 c0.  Returns the same six rows and the clause index of each ray."""
    f = rng.uniform(0.98, 1.0, (4, n))
    hd = rng.uniform(-180, 180, (4, n)); lon = rng.uniform(-125, -70, (4, n)) if lcc else rng.uniform(-170, 170, (4, n))
    sgn = np.ones((4, n)) if lcc else rng.choice([-1.0, 1.0], (4, n))
    ht = rng.choice([0., -100., 3000.], (4, n))
    out = []
    # 0: the angular travel limit, 80 km top
    zref = np.full(n, 80000.0)
    gam = M.ANG_TRAVEL_MAX * f[0]
    out.append((rng.uniform(20, 60, n) * sgn[0], np.degrees(np.arccos((zref - ht[0]) / (6.3e6 * gam))), zref))
    # 1: the longitude travel limit: c0 = gam + gam / (limit f)
    zref = rng.choice([40000., 80000.], n)
    inc = rng.uniform(30, 75, n)
    gam = (zref - ht[1]) / (6.3e6 * np.cos(np.radians(inc)))
    out.append((np.degrees(np.arccos(np.minimum(gam + gam / (M.LON_TRAVEL_MAX * f[1]), 1.0))) * sgn[1], inc, zref))
    # 2: the pole margin: c0 = gam + 0.02 / f (the shortest rays only - a 15 km top seen from 3000 m at less than 35 degrees: beyond
    # gam = 0.02 x the longitude limit that clause bites first)
    zref = np.full(n, 15000.0)
    ht[2] = 3000.0
    inc = rng.uniform(0, 35, n)
    gam = (zref - ht[2]) / (6.3e6 * np.cos(np.radians(inc)))
    out.append((np.degrees(np.arccos(gam + M.POLE_MARGIN / f[2])) * sgn[2], inc, zref))
    # 3: the cone's limit gam = 0.09 c0 f (lon/lat cubes: once more the longitude limit, at the other tops)
    if lcc:
        lat = rng.uniform(68, 80, n)             # (below 67 degrees the angular travel limit bites first)
        zref = np.full(n, 80000.0)
        gam = M.LCC_TRAVEL_MAX * np.cos(np.radians(lat)) * f[3]
        out.append((lat, np.degrees(np.arccos((zref - ht[3]) / (6.3e6 * gam))), zref))
    else:
        zref = np.full(n, 15000.0)
        inc = rng.uniform(60, 85, n)
        gam = (zref - ht[3]) / (6.3e6 * np.cos(np.radians(inc)))
        out.append((np.degrees(np.arccos(np.minimum(gam + gam / (M.LON_TRAVEL_MAX * f[3]), 1.0))) * sgn[3], inc, zref))
    lat, inc, zref = (np.concatenate([o[k] for o in out]) for k in range(3))
    return np.stack([lat, lon.ravel(), inc, hd.ravel(), zref, ht.ravel()]), np.repeat(np.arange(4), n)


def _converged_height(x, y, z):
    """height above the ellipsoid with an iterated latitude, in extended precision"""
    pp = np.sqrt(x * x + y * y)
    phi = np.arctan2(z, pp * (1 - M.WGS84_ES))
    for _ in range(6):
        n = M.WGS84_A / np.sqrt(1 - M.WGS84_ES * np.sin(phi) ** 2)
        phi = np.arctan2(z, pp * (1 - M.WGS84_ES * n / (n + (pp / np.cos(phi) - n))))
    return pp * np.cos(phi) + z * np.sin(phi) - M.WGS84_A * np.sqrt(1 - M.WGS84_ES * np.sin(phi) ** 2)


def _sweep(rows, proj):
    """the admitted rays of `rows`: per ray the worst distance of the model's three polynomials from the reference over NPTS points of
    the ray's parameter range, in metres, and everything the other tests need"""
    lat, lon, inc, hd, zref, ht = rows
    los = O.look_vectors_from_inc_hd(inc, hd, lat, lon, ht)
    ok = np.zeros(lat.size, dtype=bool)
    for zr in np.unique(zref):
        m = zref == zr
        ok[m] = M.classify(lat[m], lon[m], los[m], ht[m], zr, proj, np.array([-180.0, 180.0]))
    lat, lon, inc, zref, ht, los = lat[ok], lon[ok], inc[ok], zref[ok], ht[ok], los[ok]
    n = lat.size
    eh, ela, elo, tb = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    parts_all = {}
    for zr in np.unique(zref):
        m = np.flatnonzero(zref == zr)
        parts = {}
        q = M.fit(lat[m], lon[m], los[m], ht[m], zr, proj=proj, parts=parts)
        for k, v in parts.items():
            parts_all.setdefault(k, []).append(np.asarray(v).ravel())
        u = np.linspace(-1.0, 1.0, NPTS).astype(LD)
        t = q['mid'][:, None] + q['half'][:, None] * u[None, :]
        x, y, z = (q['o'][:, None, k] + t * q['l'][:, None, k] for k in range(3))
        rlon, rlat, _ = O.ecef2lla(x.astype(np.float64), y.astype(np.float64), z.astype(np.float64))
        eh[m] = np.abs(M.polyval(q['h'], u[None, :] * np.ones((m.size, 1), dtype=LD)) - _converged_height(x, y, z)).max(-1)
        plat, plon = (M.polyval(q[k], u[None, :] * np.ones((m.size, 1), dtype=LD)).astype(np.float64) for k in ('lat', 'lon'))
        if proj is not None:
            rx, ry = O.lcc_forward(rlat, rlon, **proj)
            ela[m], elo[m] = np.abs(plat - ry).max(-1), np.abs(plon - rx).max(-1)
        else:
            c0 = np.maximum(np.cos(np.radians(lat[m])), 0.01)
            dl = (plon - rlon + 180.0) % 360.0 - 180.0
            ela[m] = np.abs(np.radians(plat - rlat)).max(-1) * 6.4e6
            elo[m] = np.abs(np.radians(dl)).max(-1) * 6.4e6 * c0
        tb[m] = (q['mid'] + q['half']).astype(np.float64)
    return dict(n=n, ok=ok, lat=lat, lon=lon, inc=inc, zref=zref, ht=ht, los=los, eh=eh, elat=ela, elon=elo, tb=tb,
                parts={k: np.concatenate(v) for k, v in parts_all.items()})


_memo = {}


def _sweeps(kind):
    """'lonlat' / 'lcc': (random rays, edge rays, clause of each admitted edge ray)"""
    if kind not in _memo:
        rng = np.random.default_rng(SEED)
        proj = LCC if kind == 'lcc' else None
        rows = _probe_rays(N_RANDOM, rng)
        if proj is not None:                   # the cone's own region: HRRR's domain
            rows[0] = 21.0 + (rows[0] + 89.5) * (32.0 / 179.0); rows[1] = -125.0 + (rows[1] + 170.0) * (55.0 / 340.0)
        edge, clause = _edge_rays(N_EDGE, rng, lcc=proj is not None)
        a, b = _sweep(rows, proj), _sweep(edge, proj)
        _memo[kind] = (a, b, clause[b['ok']])
    return _memo[kind]


def _worst(kind, key, short=False):
    a, b, _ = _sweeps(kind)
    v = np.concatenate([a[key], b[key]])
    if short:
        v = v[np.concatenate([a['tb'], b['tb']]) < 100e3]
    return float(v.max())


# ---- a. the model against the reference over the admitted region ---------------------------------------------------------------------------


def test_the_sweep_covers_the_admitted_region_and_its_edges():
    a, b, clause = _sweeps('lonlat')
    assert a['n'] >= 2000 and b['n'] >= 500, (a['n'], b['n'])
    assert all((clause == k).sum() >= 100 for k in range(4)), np.bincount(clause, minlength=4)
    # every admitted edge ray is within 2 % of the limit of the clause it was placed at
    cosi, _, gam, c0, _ = (np.asarray(v, dtype=np.float64) for v in M.ray_frame(b['lat'], b['lon'], b['los'], b['ht'], b['zref']))
    ratio = np.select([clause == 0, (clause == 1) | (clause == 3), clause == 2],
                      [gam / M.ANG_TRAVEL_MAX, gam / (M.LON_TRAVEL_MAX * (c0 - gam)), M.POLE_MARGIN / (c0 - gam)])
    assert (ratio > 0.9799).all() and (ratio < 1.0).all(), (ratio.min(), ratio.max())
    al, bl, cl = _sweeps('lcc')
    assert al['n'] >= 2000 and (cl == 3).sum() >= 100, (al['n'], np.bincount(cl, minlength=4))


@pytest.mark.parametrize('kind', ['lonlat', 'lcc'])
def test_interpolants_against_the_reference_geodesy(kind):
    got = {(key, short): _worst(kind, key, short) for key in ('eh', 'elat', 'elon') for short in (False, True)}
    print(f'RAYBOUNDS {kind} seed {SEED}: ' + ' '.join(f'{k}{"<100km" if s else ""}={v:.2e}' for (k, s), v in got.items()))
    for key, bound in (('eh', BOUND_H), ('elat', BOUND_LAT), ('elon', BOUND_LON)):
        assert got[key, False] <= bound[0], (kind, key, got[key, False], bound[0])
        assert got[key, True] <= bound[1], (kind, key, 'rays shorter than 100 km', got[key, True], bound[1])


def _crossing_cases(kind):
    """per (zref, ht) group of the lon/lat sweep: the model's fit, crossings with and without the crossing polynomial, and the
    reference's crossings (ray parameter)"""
    key = ('crossings', kind)
    if key in _memo:
        return _memo[key]
    a, b, _ = _sweeps(kind)
    lat, lon, inc, zref, ht, los = (np.concatenate([a[k], b[k]]) for k in ('lat', 'lon', 'inc', 'zref', 'ht', 'los'))
    out = []
    for zr in np.unique(zref):
        for h0 in np.unique(ht):
            m = np.flatnonzero((zref == zr) & (ht == h0))
            if not m.size:
                continue
            zs = np.round(-100 + (zr + 1 + 100) * np.linspace(0, 1, 24) ** 2, 3)
            q = M.fit(lat[m], lon[m], los[m], h0, zr)
            cx, c3 = M.crossings(q, zs, h0, zr), M.crossings(q, zs, h0, zr, use_xpoly=False)
            xyz = np.stack(O.lla2ecef(lat[m], lon[m], np.full(m.size, h0)), -1)
            _, lows, highs = O.build_ray(zs, h0, xyz, los[m], zr)
            tref = np.concatenate([((lows[:1] - xyz) * los[m]).sum(-1), ((highs - xyz) * los[m]).sum(-1)]).T / (los[m] ** 2).sum(-1)[:, None]
            out.append(dict(q=q, cx=cx, c3=c3, tref=tref, inc=inc[m], zref=zr))
    _memo[key] = out
    return out


def test_crossings_against_the_reference():
    """the kernels' height is the exact one, the reference's (PROJ's p / cos(phi) - N on the single-pass latitude) is off it by up to
    1.7e-5 m at 40 km: the model's crossings sit that far from the reference's, measured as height (along the ray x cos(inc))"""
    worst = {}
    for g in _crossing_cases('lonlat'):
        q, cx = g['q'], g['cx']
        t = ((cx['u'] - q['ou'][:, None]) / q['su'][:, None]).astype(np.float64)
        d = np.abs(t - g['tref']) * (q['nl'] * q['cosi']).astype(np.float64)[:, None]
        worst[g['zref']] = max(worst.get(g['zref'], 0.0), float(d.max()))
    print('RAYBOUNDS crossings, metres of height from the reference by model top: ' + ' '.join(f'{z:.0f}:{v:.2e}' for z, v in worst.items()))
    assert set(worst) == set(BOUND_CROSSING) and all(worst[z] <= BOUND_CROSSING[z] for z in worst), worst


def test_crossing_polynomial_against_the_three_step_iteration():
    worst = [0.0] * len(BOUND_XPOLY)
    for g in _crossing_cases('lonlat'):
        if g['zref'] != 80000.0:
            continue
        d = (np.abs(g['cx']['u'] - g['c3']['u']) * g['q']['scale'][:, None]).astype(np.float64).max(-1)
        for i, (inc_max, _) in enumerate(BOUND_XPOLY):
            m = g['inc'] <= inc_max
            if m.any():
                worst[i] = max(worst[i], float(d[m].max()))
    print('RAYBOUNDS crossing polynomial - three steps, m along the ray, 80 km top: ' + ' '.join(f'<={b[0]:.0f}deg:{w:.2e}' for b, w in zip(BOUND_XPOLY, worst)))
    assert all(w > 0 for w in worst)
    for (inc_max, bound), w in zip(BOUND_XPOLY, worst):
        assert w <= bound, (inc_max, w, bound)


# ---- b. series truncations ------------------------------------------------------------------------------------------------------------------


def test_asin_series_truncation():
    a, b, _ = _sweeps('lonlat')
    s = np.concatenate([a['parts']['sd'], a['parts']['sl'], b['parts']['sd'], b['parts']['sl']])
    d = float(np.abs(M.asin_small(s) - np.arcsin(s)).max())
    print(f'RAYBOUNDS asin series: largest argument {float(np.abs(s).max()):.4f}, truncation {d:.2e} rad')
    assert np.abs(s).max() > 0.75 * M.LON_TRAVEL_MAX and d <= BOUND_ASIN, d


def test_lcc_series_truncations():
    a, b, _ = _sweeps('lcc')
    zz, xe, ang = (np.concatenate([a['parts'][k], b['parts'][k]]) for k in ('zz', 'xe', 'ang'))
    n = M.lcc_params(LCC)['n']
    em1, sn, cm, xs = M.lcc_series(zz, ang, n)
    eps = np.finfo(LD).eps
    zmax, xmax, amax = (float(np.abs(v).max()) for v in (zz, xe, ang))
    nxt = (zmax ** 10 / 11, xmax ** 9 / float(M._fact(10)), amax ** 12 / float(M._fact(13)))
    print(f'RAYBOUNDS lcc series: |z| <= {zmax:.4f} |x| <= {xmax:.4f} |angle| <= {amax:.4f}; next terms {nxt[0]:.1e} {nxt[1]:.1e} {nxt[2]:.1e}')
    assert zmax < 0.05 and amax < 0.2
    for got, bound in zip(nxt, BOUND_LCC_SERIES):
        assert got <= bound, (nxt, BOUND_LCC_SERIES)
    nz = zz != 0
    assert (np.abs(xs[nz] / (2 * n * np.arctanh(zz[nz])) - 1)).max() <= BOUND_LCC_SERIES[0] + 4 * eps
    assert (np.abs(em1[nz] / np.expm1(xe[nz]) - 1)).max() <= BOUND_LCC_SERIES[1] + 4 * eps
    na = ang != 0
    assert (np.abs(sn[na] / np.sin(ang[na]) - 1)).max() <= BOUND_LCC_SERIES[2] + 4 * eps
    assert np.abs(cm - (-2 * np.sin(ang / 2) ** 2)).max() <= BOUND_LCC_SERIES[2] + 4 * eps


# ---- the interpolation matrices of the headers ------------------------------------------------------------------------------------------------


def _table(text, name):
    body = re.search(name + r'\[\w+\]\[\w+\]\s*=\s*\{(.*?)\};', text, re.S).group(1)
    body = re.sub(r'//[^\n]*', '', body)
    rows = re.findall(r'\{([^{}]*)\}', body)
    return np.array([[float(v) for v in r.split(',')] for r in rows])


def _nodes(text, name):
    return np.array([float(v) for v in re.search(name + r'\[\w+\]\s*=\s*\{(.*?)\};', text, re.S).group(1).split(',')])


@pytest.mark.parametrize('header,nodes,table,ref_nodes,ref', [('geodesy_fast.h', 'RAY_POLY_NODES', 'RAY_POLY_VINV', M.NODES5, M.VINV5),
                                                            ('raider_kernels.h', 'XPOLY_NODES', 'XPOLY_VINV', M.NODES7, M.VINV7)])
def test_interpolation_tables_of_the_headers(header, nodes, table, ref_nodes, ref):
    """every entry of the kernels' node and inverse-Vandermonde tables is the double nearest to the value derived from the node formula"""
    text = (CSRC / header).read_text()
    assert np.array_equal(_nodes(text, nodes), ref_nodes.astype(np.float64))
    got = _table(text, table)
    assert got.shape == ref.shape and np.array_equal(got, ref.astype(np.float64)), np.abs(got - ref.astype(np.float64)).max()
