"""The light ray geometry of the two ray passes, restated in extended precision (a helper, not a test).

Per ray the kernels evaluate a cheap ECEF -> geodetic at six Chebyshev nodes of the ray's parameter range, fit degree-5 polynomials
for height, latitude and longitude (or Lambert-conic northing and easting), and find every level crossing by Newton steps on the
height polynomial, folded into a degree-7 crossing polynomial (raider_amd/csrc/geodesy_fast.h, raider_kernels.h: crossings_kernel,
fit_crossing_poly, march_slice_levels).  This module restates that DESIGN - not the device's instruction sequences - in np.longdouble,
vectorised over rays: exact 1/sqrt and sqrt where the device has a reciprocal-square-root seed with one Newton-Raphson step and a
Taylor polynomial, and the interpolation matrices from the node formula where the device has tables.  What the device adds to this
model is rounding; what the model adds to the reference's geodesy is the documented design error.
tests/test_ray_poly_bounds.py pins the second on the CPU, tests/test_gpu_ray_geometry.py the first on the device.

Nothing is imported from the package or from the compiled library; the constants are those of csrc/geodesy.h."""
import numpy as np

LD = np.longdouble
WGS84_A = LD(6378137.0)
_F = 1.0 / 298.257223563                        # (the constants are the kernels' doubles, widened)
_ES = 2.0 * _F - _F * _F
WGS84_ES = LD(_ES)
WGS84_B = LD((1.0 - _F) * 6378137.0)
WGS84_E2S = LD(_ES / (1.0 - _ES))
PI = LD('3.14159265358979323846264338327950288')
D2R = PI / 180
R2D = 180 / PI
PN, PX = 6, 8
LON_TRAVEL_MAX, ANG_TRAVEL_MAX, POLE_MARGIN, LCC_TRAVEL_MAX, COSI_MIN = 0.12, 0.035, 0.02, 0.09, 0.05


def ld(a):
    return np.asarray(a, dtype=LD)


def cheb_nodes(n):
    """u_j = cos(pi (2j+1) / (2n)), descending"""
    return np.cos(PI * (2 * ld(np.arange(n)) + 1) / (2 * n))


def inverse_vandermonde(u):
    """M[j][n]: coefficient of u^n in the Lagrange basis polynomial of node j, so that c[n] = sum_j M[j][n] f(u_j)"""
    n = u.size
    M = np.zeros((n, n), dtype=LD)
    for j in range(n):
        p = np.zeros(n, dtype=LD); p[0] = 1
        den = LD(1)
        for m in range(n):
            if m == j:
                continue
            p = np.concatenate([[LD(0)], p[:-1]]) - u[m] * p          # p * (u - u_m)
            den = den * (u[j] - u[m])
        M[j] = p / den
    return M


NODES5, NODES7 = cheb_nodes(PN), cheb_nodes(PX)
VINV5, VINV7 = inverse_vandermonde(NODES5), inverse_vandermonde(NODES7)


def polyval(c, u):
    """c[..., n] monomial coefficients (ascending), u[...] or u[..., m]"""
    c = ld(c); u = ld(u)
    extra = u.ndim - (c.ndim - 1)
    r = c[..., -1].reshape(c.shape[:-1] + (1,) * extra) * np.ones_like(u)
    for n in range(c.shape[-1] - 2, -1, -1):
        r = r * u + c[..., n].reshape(c.shape[:-1] + (1,) * extra)
    return r


# ---- static classification (raider_kernels.h: fast_ok) --------------------------------------------------------------------------------


def ray_frame(lat, lon, los, hts, zref):
    """cos of the incidence at the origin, |l|, gam, cos(lat) - the quantities the clauses of fast_ok compare"""
    la, lo = ld(lat).ravel() * D2R, ld(lon).ravel() * D2R
    l = ld(los).reshape(-1, 3)
    nl = np.sqrt((l * l).sum(-1))
    up = np.stack([np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)], -1)
    cosi = (l * up).sum(-1) / nl
    hti = ld(hts).ravel() if np.size(hts) == la.size else np.broadcast_to(ld(hts), la.shape)
    gam = (LD(zref) - hti) / (cosi * LD(6.3e6))
    return cosi, nl, gam, np.cos(la), hti


def classify(lat, lon, los, hts, zref, proj=None, xs=None):
    """True where the static classification admits the ray to the polynomial (light) path.  proj: None (lon/lat cube with x axis xs)
    or the cone's parameters (dict with lon_0 and es)."""
    cosi, _, gam, c0, _ = ray_frame(lat, lon, los, hts, zref)
    lon = np.asarray(lon, dtype=np.float64).ravel()
    if proj is not None:
        dl = lon - proj['lon_0']
        dl = dl - 360.0 * np.rint(dl / 360.0)
        ok = (np.abs(dl) + 12.0 < 180.0) & (proj.get('es', 0.0) == 0.0) & (gam < LCC_TRAVEL_MAX * c0)
    else:
        xs = np.asarray(xs, dtype=np.float64)
        wrap_pos = xs.max() <= 180.0 and xs.min() > -168.0
        wrap_neg = xs.min() >= -180.0 and xs.max() < 168.0
        ok = (np.abs(lon) + 5.0 < 180.0) | ((np.abs(lon) <= 180.0) & np.where(lon > 0.0, wrap_pos, wrap_neg))
    return (cosi > COSI_MIN) & (c0 > gam + POLE_MARGIN) & (gam < LON_TRAVEL_MAX * (c0 - gam)) & (gam < ANG_TRAVEL_MAX) & ok


# ---- node geodesy (geodesy_fast.h) -------------------------------------------------------------------------------------------------------


def lla2ecef(lat, lon, h):
    la, lo, h = ld(lat) * D2R, ld(lon) * D2R, ld(h)
    s, c = np.sin(la), np.cos(la)
    N = WGS84_A / np.sqrt(1 - WGS84_ES * s * s)
    return np.stack([(N + h) * c * np.cos(lo), (N + h) * c * np.sin(lo), (N * (1 - WGS84_ES) + h) * s], -1)


def geo_fast(x, y, z):
    """(p, sin phi, cos phi, h): the single-pass Bowring latitude and the support-function height"""
    p = np.sqrt(x * x + y * y)
    xt, yt = p * WGS84_B, z * WGS84_A
    rn = 1 / np.sqrt(xt * xt + yt * yt)
    c, s = xt * rn, yt * rn
    y_phi = z + WGS84_E2S * WGS84_B * s * s * s
    x_phi = p - WGS84_ES * WGS84_A * c * c * c
    r = 1 / np.sqrt(x_phi * x_phi + y_phi * y_phi)
    sphi, cphi = y_phi * r, x_phi * r
    h = p * cphi + z * sphi - WGS84_A * np.sqrt(1 - WGS84_ES * sphi * sphi)
    return p, sphi, cphi, h


ASIN_COEF = (LD(1) / 6, LD(3) / 40, LD(5) / 112, LD(35) / 1152, LD(63) / 2816)           # s^3 .. s^11


def asin_small(s, terms=5):
    """the odd series through s^(2 terms + 1) (the kernels: terms = 5, through s^11)"""
    s2 = s * s
    q = np.zeros_like(s)
    for c in ASIN_COEF[:terms][::-1]:
        q = q * s2 + c
    return s * s2 * q + s


def make_base(lat, lon):
    la, lo = ld(lat) * D2R, ld(lon) * D2R
    return dict(lat0=ld(lat), lon0=ld(lon), s0=np.sin(la), c0=np.cos(la), sl0=np.sin(lo), cl0=np.cos(lo))


def ecef2lla_delta(b, x, y, z, series=True, asin_terms=5, parts=None):
    """(lon - lon0, lat - lat0) in degrees and h.  b's entries broadcast against x, y, z.  parts: a dict that receives the two sines."""
    p, sphi, cphi, h = geo_fast(x, y, z)
    sd = sphi * b['c0'] - cphi * b['s0']
    sl = (b['cl0'] * y - b['sl0'] * x) / p
    if parts is not None:
        parts.update(sd=sd, sl=sl)
    if series:
        return asin_small(sl, asin_terms) * R2D, asin_small(sd, asin_terms) * R2D, h
    return np.arcsin(sl) * R2D, np.arcsin(sd) * R2D, h


def lcc_params(proj):
    """n, a F, rho0, lam0, x0, y0 of a spherical cone (geodesy.h: lcc_setup with es = 0)"""
    assert proj.get('es', 0.0) == 0.0, 'the light path projects spherical cones only'
    p1, p2, p0 = (LD(proj[k]) * D2R for k in ('lat_1', 'lat_2', 'lat_0'))

    def ts(phi):
        return np.tan((PI / 2 - phi) / 2)
    n = np.log(np.cos(p1) / np.cos(p2)) / np.log(ts(p1) / ts(p2)) if abs(p1 - p2) >= 1e-10 else np.sin(p1)
    aF = LD(proj.get('a', 6371229.0)) * np.cos(p1) * ts(p1) ** (-n) / n
    return dict(n=n, aF=aF, rho0=aF * ts(p0) ** n, lam0=LD(proj['lon_0']) * D2R, x0=LD(proj.get('x_0', 0.0)), y0=LD(proj.get('y_0', 0.0)))


def lcc_origin(L, b):
    """rho, sin theta, cos theta of the ray origins (geodesy_fast.h: lcc_rho, lcc_theta)"""
    rho = L['aF'] * np.exp(L['n'] * np.log(b['c0'] / (1 + b['s0'])))
    dlam = b['lon0'] * D2R - L['lam0']
    dlam = np.where(dlam > PI, dlam - 2 * PI, np.where(dlam < -PI, dlam + 2 * PI, dlam))
    return dict(rho=rho, st=np.sin(L['n'] * dlam), ct=np.cos(L['n'] * dlam))


def _fact(k):
    r = LD(1)
    for i in range(2, k + 1):
        r = r * i
    return r


def lcc_series(zz, ang, n):
    """(exp(n 2 atanh zz) - 1, sin ang, cos ang - 1) by the kernels' series: atanh through z^9, exp through x^9, sin / cos through
    x^11 / x^12"""
    z2 = zz * zz
    q = z2 * LD(1) / 9 + LD(1) / 7
    q = q * z2 + LD(1) / 5
    q = q * z2 + LD(1) / 3
    xe = n * (2 * (zz * z2 * q + zz))
    e = np.zeros_like(xe)
    for k in range(9, 0, -1):
        e = e * xe + 1 / _fact(k)
    em1 = xe * e
    a2 = ang * ang
    sn = np.zeros_like(ang)
    for k in (11, 9, 7, 5, 3):
        sn = sn * a2 + (-1) ** ((k - 1) // 2) / _fact(k)
    sn = ang * a2 * sn + ang
    cm = np.zeros_like(ang)
    for k in (12, 10, 8, 6, 4, 2):
        cm = cm * a2 + (-1) ** (k // 2) / _fact(k)
    return em1, sn, a2 * cm, xe


def ecef2lcc_sphere(b, L, org, x, y, z, series=True, asin_terms=5, parts=None):
    """(x - x_origin, y - y_origin) on the cone and h.  parts: a dict that receives zz, xe and ang (the series' arguments)."""
    p, sphi, cphi, h = geo_fast(x, y, z)
    sl = (b['cl0'] * y - b['sl0'] * x) / p
    ta, tb = cphi * (1 + b['s0']), b['c0'] * (1 + sphi)
    zz = (ta - tb) / (ta + tb)
    if series:
        ang = L['n'] * asin_small(sl, asin_terms)
        em1, sn, cm, xe = lcc_series(zz, ang, L['n'])
    else:
        ang = L['n'] * np.arcsin(sl)
        xe = L['n'] * 2 * np.arctanh(zz)
        em1, sn, cm = np.expm1(xe), np.sin(ang), -2 * np.sin(ang / 2) ** 2
    if parts is not None:
        parts.update(zz=zz, xe=xe, ang=ang, sl=sl)
    ds, dc = org['st'] * cm + org['ct'] * sn, org['ct'] * cm - org['st'] * sn
    return org['rho'] * (em1 * (org['st'] + ds) + ds), -org['rho'] * (em1 * (org['ct'] + dc) + dc), h


# ---- the ray polynomials (geodesy_fast.h: fit_ray_poly; raider_kernels.h: the range [t_a, t_b]) --------------------------------------------


def fit(lat, lon, los, hts, zref, proj=None, xyz=None, series=True, asin_terms=5, vinv=None, parts=None):
    """The polynomials of n rays: dict with h, lat, lon [n, 6] (monomial in u; lat / lon in degrees, or northing / easting in metres
    on a cone), su, ou (u = su t + ou), half, mid, nl (|l|), scale (metres per unit of u), o [n, 3], l [n, 3], cosi, hti.
    xyz: ECEF origins (default: lla2ecef(lat, lon, hts)); lat / lon are then the frame the kernel derives from them.
    vinv: another interpolation matrix [node][power] (default: the inverse Vandermonde matrix of the nodes)."""
    cosi, nl, _, _, hti = ray_frame(lat, lon, los, hts, zref)
    lat, lon = ld(lat).ravel(), ld(lon).ravel()
    l = ld(los).reshape(-1, 3)
    o = lla2ecef(lat, lon, hti) if xyz is None else ld(xyz).reshape(-1, 3)
    zref = LD(zref)
    t_end = (zref - hti) / (cosi * nl)
    t_a = np.minimum(np.minimum(LD(0), hti), t_end) - 1
    t_b = np.maximum(np.maximum(zref, hti), t_end) + 1
    half, mid = (t_b - t_a) / 2, (t_b + t_a) / 2
    su = 1 / half
    ou = -mid * su
    b = make_base(lat, lon)
    t = mid[:, None] + half[:, None] * NODES5[None, :]                                  # [n, 6]
    x, y, z = (o[:, None, k] + t * l[:, None, k] for k in range(3))
    bb = {k: v[:, None] for k, v in b.items()}
    if proj is not None:
        L = lcc_params(proj)
        org = lcc_origin(L, b)
        dx, dy, h = ecef2lcc_sphere(bb, L, {k: v[:, None] for k, v in org.items()}, x, y, z, series, asin_terms, parts)
        x0, y0 = org['rho'] * org['st'] + L['x0'], L['y0'] + L['rho0'] - org['rho'] * org['ct']
    else:
        dx, dy, h = ecef2lla_delta(bb, x, y, z, series, asin_terms, parts)
        x0, y0 = b['lon0'], b['lat0']
    V = VINV5 if vinv is None else ld(vinv)
    q = dict(h=h @ V, lat=dy @ V, lon=dx @ V)
    q['lat'][:, 0] += y0
    q['lon'][:, 0] += x0
    q.update(su=su, ou=ou, half=half, mid=mid, nl=nl, scale=nl * half, o=o, l=l, cosi=cosi, hti=hti)
    return q


# ---- level crossings (raider_kernels.h: crossings_kernel, fit_crossing_poly, fill_levels, first_level) --------------------------------------


def level_table(zs, ht, zref):
    """(lo, hi, kz) of build_ray's slice-uniform level table (raider_kernels.h: build_levels)"""
    zs = np.asarray(zs, dtype=np.float64)
    lo, hi, kz = [], [], []
    for zz in range(zs.size - 1):
        a, b = zs[zz], zs[zz + 1]
        if b == zs[-1]:
            b = b - 0.01
        if b < ht or a >= zref:
            continue
        a, b = max(a, ht), min(b, zref)
        if abs(b - a) < 1.0:
            continue
        lo.append(a); hi.append(b); kz.append(zz)
    return np.array(lo), np.array(hi), np.array(kz, dtype=int)


def first_level(zs, lo, hi, kz, hti):
    """per ray: (k0, lo_first) - the first level of the table the ray contributes to (K: none) and its clipped bottom"""
    zs = np.asarray(zs, dtype=np.float64)
    hti = np.asarray(hti, dtype=np.float64).ravel()
    K = lo.size
    raw_top = zs[kz + 1] - np.where(zs[kz + 1] == zs[-1], 0.01, 0.0)
    k0 = np.full(hti.size, K); lo_first = np.zeros(hti.size)
    for i, h in enumerate(hti):
        for k in range(K):
            if raw_top[k] < h:
                continue
            b = max(lo[k], h)
            if abs(hi[k] - b) < 1.0:
                continue
            k0[i], lo_first[i] = k, b
            break
    return k0, lo_first


def crossing_range(hi):
    """hm, hh: centre and half width of the level-top range the crossing polynomial covers (fill_levels)"""
    K = hi.size
    a = hi[1] if K > 1 else (hi[0] if K > 0 else 0.0)
    b = hi[K - 1] if K > 1 else a
    return LD(0.5) * (LD(a) + LD(b)), np.maximum(LD(0.5) * (LD(b) - LD(a)), LD(1))


def three_step(q, h, gain):
    """getTopOfAtmosphere's three iterations on u from u0 = u(t = h), with the ray's height polynomial; h: [n, m]"""
    u = h * q['su'][:, None] + q['ou'][:, None]
    for _ in range(3):
        u = u + (h - polyval(q['h'], u)) * gain[:, None]
    return u


def crossings(q, zs, ht, zref, per_ray=False, use_xpoly=True, vinv=None):
    """Level crossings of every ray on the table of slice height ht (per_ray: the table of the lowest ray, each ray joining it at its
    own first level with its own height q['hti']).  Returns dict: u [n, K + 1] (u[:, k] bottom of level k, u[:, k + 1] its top; NaN
    below a ray's first level), L [n, K] lengths in metres (0 below the first level), k0 [n], lo, hi, kz, xc [n, 8], gain."""
    lo, hi, kz = level_table(zs, ht, zref)
    K, n = lo.size, q['su'].size
    if per_ray:
        k0, lo_first = first_level(zs, lo, hi, kz, q['hti'])
    else:
        k0, lo_first = np.zeros(n, dtype=int), np.full(n, lo[0])
    assert (k0 < K).all(), 'a ray without any level'
    lo1, hi1 = ld(lo_first), ld(hi[k0])
    u_lo, u_hi = lo1 * q['su'] + q['ou'], hi1 * q['su'] + q['ou']
    for _ in range(10):
        u_lo = u_lo + (lo1 - polyval(q['h'], u_lo)) * q['su']
        u_hi = u_hi + (hi1 - polyval(q['h'], u_hi)) * q['su']
    L0 = np.abs(u_hi - u_lo) * q['scale']
    gain = q['su'] * (L0 / (hi1 - lo1))
    hm, hh = crossing_range(hi)
    un = three_step(q, (hh * NODES7 + hm)[None, :] * np.ones((n, 1), dtype=LD), gain)
    xc = un @ (VINV7 if vinv is None else ld(vinv))
    if use_xpoly:
        tops = polyval(xc, np.broadcast_to(((ld(hi) - hm) / hh)[None, :], (n, K)))
    else:
        tops = three_step(q, np.broadcast_to(ld(hi)[None, :], (n, K)), gain)
    u = np.full((n, K + 1), np.nan, dtype=LD)
    Ls = np.zeros((n, K), dtype=LD)
    for i in range(n):
        k = k0[i]
        u[i, k], u[i, k + 1] = u_lo[i], u_hi[i]
        u[i, k + 2:] = tops[i, k + 1:]
    kk = np.arange(K)[None, :]
    Ls = np.where(kk >= k0[:, None], np.abs(u[:, 1:] - u[:, :-1]) * q['scale'][:, None], LD(0))
    return dict(u=u, L=Ls, k0=k0, lo=lo, hi=hi, kz=kz, xc=xc, gain=gain, hm=hm, hh=hh)


def maxlen(cr, counts=None):
    """per-level maximum of the lengths over the rays that count (default: all)"""
    L = (cr['L'] if counts is None else cr['L'][np.asarray(counts).ravel()]).astype(np.float64)
    return np.fmax(L, 0.0).max(0) if L.shape[0] else np.zeros(cr['lo'].size)


def path_sum(q, cr, nparts, integrand):
    """Pass 2's trapezoid sum of integrand(us) -> values [n, nParts] at the samples us = u_k + f du, f = i / (nParts - 1), of every
    level k: weights L 1e-6 / (nParts - 1), half of that at the two ends.  Returns the sum [n]."""
    n, K = cr['L'].shape
    out = np.zeros(n, dtype=LD)
    for k in range(K):
        live = cr['k0'] <= k
        npk = int(nparts[k])
        if npk < 2 or not live.any():
            continue
        f = ld(np.arange(npk)) / (npk - 1)
        f[-1] = 1
        ua, ub = cr['u'][:, k], cr['u'][:, k + 1]
        v = ld(integrand(ua[:, None] + f[None, :] * (ub - ua)[:, None]))
        w = np.full(npk, LD(1)); w[0] = w[-1] = LD(0.5)
        seg = (v * w[None, :]).sum(-1) * (LD(1e-6) * cr['L'][:, k] / (npk - 1))
        out = out + np.where(live, seg, LD(0))
    return out


def sample_points(q, us):
    """ECEF x, y, z of the samples at us [n, m] of every ray"""
    t = (us - q['ou'][:, None]) / q['su'][:, None]
    return tuple(q['o'][:, None, k] + t * q['l'][:, None, k] for k in range(3))


def linear_field_delay(q, cr, nparts, coord, centre=0.0, scale=1.0):
    """Pass 2's trapezoid sum for a field scale * (coordinate - centre), coordinate = 'lat', 'lon' or 'h' (the value of that
    polynomial at the sample): per level k with nParts[k] samples at u_k + f du, f = i / (nParts - 1), weights L 1e-6 / (nParts - 1),
    half of that at the two ends.  Returns (delay [n], sum of the lengths [n])."""
    return path_sum(q, cr, nparts, lambda us: (polyval(q[coord], us) - LD(centre)) * LD(scale)), cr['L'].sum(-1)
