"""Anchors for the zero-Doppler solver that neither the builder's oracle nor its kernel had a hand in (isce3 is absent):

* a CIRCULAR orbit in the equatorial plane, S(t) = r (cos wt, sin wt, 0), V = dS/dt (the geometry of the reference's
  test/fake_raytracing:73-111, with velocities consistent with the positions).  For ANY target T the zero-Doppler condition
  (S - T) . V = 0 reduces to T . V = 0 (S . V = 0 on a circle), i.e. sin(lon_T - w t) = 0: the azimuth time is EXACTLY lon_T / w,
  the sensor is at the target's longitude, slant range^2 = r^2 + |T|^2 - 2 r |T| cos(geocentric latitude), and the look vector
  follows in closed form.  What remains between that and the solver is the 4-point Hermite interpolation error of a circle
  sampled every 10 s: <= (w dt)^4 / 384 r = 2e-4 m.
* the eight Sentinel-1 state vectors the reference's own test suite carries (test/test_losreader.py:20-92, from
  test/orbit_files/S1_orbit_example.EOF): Hermite interpolation through every OTHER vector must land on the skipped ones.
"""
import numpy as np

W = 2 * np.pi / 5900.0            # rad/s: a 98-minute orbit
RS = 6378137.0 + 700000.0         # test/fake_raytracing:82,89


def circular_orbit(n=41, dt=10.0):
    t = dt * np.arange(n)
    pos = np.stack([RS * np.cos(W * t), RS * np.sin(W * t), np.zeros(n)], -1)
    vel = np.stack([-RS * W * np.sin(W * t), RS * W * np.cos(W * t), np.zeros(n)], -1)
    return t, pos, vel


def targets(rng, n=500, t_lo=60.0, t_hi=340.0):
    """Targets on / near the ellipsoid whose closed-form azimuth time lies inside the orbit arc; either look side."""
    lon = W * rng.uniform(t_lo, t_hi, n)
    lat = np.radians(rng.uniform(2.0, 9.0, n)) * rng.choice([-1.0, 1.0], n)
    rad = 6378137.0 * (1 - 0.00335 * np.sin(lat) ** 2) + rng.uniform(-100.0, 9000.0, n)        # geocentric radius
    T = np.stack([rad * np.cos(lat) * np.cos(lon), rad * np.cos(lat) * np.sin(lon), rad * np.sin(lat)], -1)
    t0 = lon / W
    S = np.stack([RS * np.cos(lon), RS * np.sin(lon), np.zeros(n)], -1)
    rg = np.sqrt(RS ** 2 + rad ** 2 - 2 * RS * rad * np.cos(lat))
    los = (S - T) / rg[:, None]
    return T, t0, rg, los


# test/test_losreader.py:20-92 (seconds after 2018-11-12T23:00:02)
S1_T = np.arange(8) * 10.0
S1_POS = np.array([[-2064965.285362, 6434865.494987, 2090670.967443], [-2056228.553736, 6460407.492520, 2019650.417312],
                   [-2047224.526705, 6485212.031660, 1948401.684024], [-2037955.293282, 6509275.946120, 1876932.818066],
                   [-2028422.977002, 6532596.156540, 1805251.894958], [-2018629.735564, 6555169.670917, 1733367.014327],
                   [-2008577.760461, 6576993.585012, 1661286.298987], [-1998269.276601, 6598065.082739, 1589017.893976]])
S1_VEL = np.array([[860.239634, 2590.964968, -7090.378144], [887.072466, 2517.380329, -7113.598127], [913.698134, 2443.474728, -7136.014344],
                   [940.113169, 2369.256838, -7157.624244], [966.314136, 2294.735374, -7178.425371], [992.297636, 2219.919093, -7198.415359],
                   [1018.060311, 2144.816789, -7217.591940], [1043.598837, 2069.437298, -7235.952940]])


# ---- the extended-precision reference of the zero-Doppler solver (tests/test_gpu_orbit_solver.py) -------------------------------
# The algorithm raider_amd/csrc/orbit_kernels.h states - 4-point Hermite interpolation, Newton from the orbit mid time, threshold,
# iteration cap, in-span rule - in NumPy long double, with divisions and no tables, and with no code of the oracle module.
import collections

LD = np.longdouble
EXTENDED = np.finfo(LD).nmant >= 63            # False: the tests rerun a subsample with `decimal` (solve_decimal) and say so
PI_LD = LD(4) * np.arctan(LD(1))
Solve = collections.namedtuple('Solve', 'los t rg count margin vel')


def hermite_ld(st, sp, sv, t, shift=0):
    """orbit_hermite's literal formulas at times t.  `shift` moves the node window down by that many nodes (same clamp): only the
    window-visibility self-check passes one."""
    st, sp, sv = np.asarray(st, LD), np.asarray(sp, LD), np.asarray(sv, LD)
    t = np.atleast_1d(np.asarray(t, LD))
    n = st.size
    lo = np.searchsorted(st, t, side='right')                    # first index with t < st[idx]; n for a NaN
    i0 = np.clip(lo - 2 - shift, 0, n - 4)
    w = i0[:, None] + np.arange(4)
    tt, X, V = st[w], sp[w], sv[w]
    pos, vel = np.zeros((t.size, 3), LD), np.zeros((t.size, 3), LD)
    one, two = LD(1), LD(2)
    for i in range(4):
        oth = [j for j in range(4) if j != i]
        d = t - tt[:, i]
        ssum = np.zeros(t.size, LD)
        for j in oth:
            ssum = ssum + one / (tt[:, i] - tt[:, j])
        f0 = one - two * d * ssum
        h = np.ones(t.size, LD)
        for k in oth:
            h = h * ((t - tt[:, k]) / (tt[:, i] - tt[:, k]))
        hdot = np.zeros(t.size, LD)
        for j in oth:
            p2 = np.ones(t.size, LD)
            for k in oth:
                if k != j:
                    p2 = p2 * ((t - tt[:, k]) / (tt[:, i] - tt[:, k]))
            hdot = hdot + p2 / (tt[:, i] - tt[:, j])
        g1 = h + two * d * hdot
        g0 = two * (f0 * hdot - h * ssum)
        pos = pos + (X[:, i] * f0[:, None] + V[:, i] * d[:, None]) * (h * h)[:, None]
        vel = vel + (X[:, i] * g0[:, None] + V[:, i] * g1[:, None]) * h[:, None]
    return pos, vel


def solve_ld(st, sp, sv, xyz, threshold=1.0e-7, maxiter=30, shift=0):
    """orbit_los_kernel's iteration, literally.  Returns Solve(los, t, rg, count, margin, vel): NaN where the target is not valid
    (not converged within `maxiter` evaluations, t outside [st[0], st[-1]], a non-finite target); count = evaluations up to the
    converging one (maxiter + 1: none converged); margin = min over the iterations of | |step| / threshold - 1 |, the distance of the
    stopping rule from a tie (inf for a NaN target); vel = the sensor velocity at t."""
    st, sp, sv = np.asarray(st, LD), np.asarray(sp, LD), np.asarray(sv, LD)
    T = np.asarray(xyz, LD).reshape(-1, 3)
    m = T.shape[0]
    thr = LD(threshold)
    t = np.full(m, LD(0.5) * (st[0] + st[-1]))
    done = np.zeros(m, bool)
    count = np.full(m, maxiter + 1)
    margin = np.full(m, np.inf, LD)
    for it in range(maxiter):
        idx = np.nonzero(~done)[0]
        if idx.size == 0:
            break
        pos, vel = hermite_ld(st, sp, sv, t[idx], shift)
        d = T[idx] - pos
        fn = d[:, 0] * vel[:, 0] + d[:, 1] * vel[:, 1] + d[:, 2] * vel[:, 2]
        fnp = -(vel[:, 0] * vel[:, 0] + vel[:, 1] * vel[:, 1] + vel[:, 2] * vel[:, 2])
        step = fn / fnp
        t[idx] = t[idx] - step
        margin[idx] = np.fmin(margin[idx], np.abs(np.abs(step) / thr - 1))
        conv = np.abs(step) < thr
        count[idx[conv]] = it + 1
        done[idx[conv]] = True
    with np.errstate(invalid='ignore'):
        valid = done & (t >= st[0]) & (t <= st[-1]) & np.isfinite(T).all(-1)
    pos, vel = hermite_ld(st, sp, sv, np.where(valid, t, st[0]), shift)
    d = pos - np.where(valid[:, None], T, 0)
    rg = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    los = d / rg[:, None]
    nan = LD(np.nan)
    return Solve(np.where(valid[:, None], los, nan), np.where(valid, t, nan), np.where(valid, rg, nan), count, margin, vel)


def solve_decimal(st, sp, sv, xyz, threshold=1.0e-7, maxiter=30, digits=40):
    """solve_ld's iteration with `decimal` at `digits` digits, target by target: for a NumPy whose long double is not the 80-bit
    format.  Returns (t, rg, los) as float64 arrays (NaN where not valid)."""
    import decimal
    D = decimal.Decimal
    with decimal.localcontext() as c:
        c.prec = digits
        s_t = [D(float(x)) for x in st]
        s_p = [[D(float(x)) for x in r] for r in sp]
        s_v = [[D(float(x)) for x in r] for r in sv]
        n = len(s_t)

        def herm(t):
            lo = int(np.searchsorted(np.asarray(st, np.float64), float(t), side='right'))
            while lo > 0 and t < s_t[lo - 1]:
                lo -= 1
            while lo < n and not t < s_t[lo]:
                lo += 1
            i0 = min(max(lo - 2, 0), n - 4)
            tt = s_t[i0:i0 + 4]
            pos, vel = [D(0)] * 3, [D(0)] * 3
            for i in range(4):
                oth = [j for j in range(4) if j != i]
                d = t - tt[i]
                ssum = sum(1 / (tt[i] - tt[j]) for j in oth)
                f0 = 1 - 2 * d * ssum
                h = D(1)
                for k in oth:
                    h *= (t - tt[k]) / (tt[i] - tt[k])
                hdot = D(0)
                for j in oth:
                    p2 = D(1)
                    for k in oth:
                        if k != j:
                            p2 *= (t - tt[k]) / (tt[i] - tt[k])
                    hdot += p2 / (tt[i] - tt[j])
                g1 = h + 2 * d * hdot
                g0 = 2 * (f0 * hdot - h * ssum)
                for k in range(3):
                    pos[k] = pos[k] + (s_p[i0 + i][k] * f0 + s_v[i0 + i][k] * d) * h * h
                    vel[k] = vel[k] + (s_p[i0 + i][k] * g0 + s_v[i0 + i][k] * g1) * h
            return pos, vel
        X = np.asarray(xyz, np.float64).reshape(-1, 3)
        out_t, out_rg, out_los = np.full(X.shape[0], np.nan), np.full(X.shape[0], np.nan), np.full((X.shape[0], 3), np.nan)
        for q, row in enumerate(X):
            if not np.isfinite(row).all():
                continue
            T = [D(float(x)) for x in row]
            t = (s_t[0] + s_t[-1]) / 2
            ok = False
            for _ in range(maxiter):
                pos, vel = herm(t)
                step = sum((T[k] - pos[k]) * vel[k] for k in range(3)) / -sum(v * v for v in vel)
                t -= step
                if abs(step) < D(float(threshold)):
                    ok = True
                    break
            if ok and s_t[0] <= t <= s_t[-1]:
                pos, _ = herm(t)
                d = [pos[k] - T[k] for k in range(3)]
                rg = sum(x * x for x in d).sqrt()
                out_t[q], out_rg[q], out_los[q] = float(t), float(rg), [float(x / rg) for x in d]
        return out_t, out_rg, out_los


def lla2ecef_ld(lat, lon, h):
    """WGS84 geodetic (degrees, metres) -> ECEF, long double: (..., 3)"""
    a, f = LD(6378137), 1 / LD('298.257223563')
    e2 = f * (2 - f)
    la, lo, h = np.asarray(lat, LD) * PI_LD / 180, np.asarray(lon, LD) * PI_LD / 180, np.asarray(h, LD)
    nu = a / np.sqrt(1 - e2 * np.sin(la) ** 2)
    return np.stack(np.broadcast_arrays((nu + h) * np.cos(la) * np.cos(lo), (nu + h) * np.cos(la) * np.sin(lo), (nu * (1 - e2) + h) * np.sin(la)), -1)


def kepler_orbit(times, t0, lat0=30.5, lon0=-121.3, heading=-12.0, a=7.07e6, ecc=0.0012, nu0=1.1, wobble_m=5.0, wobble_period=50.0):
    """State vectors (float64 pos[n, 3], vel[n, 3]) of a slightly eccentric Kepler arc at the strictly increasing `times`: at t0 the
    sensor stands over (lat0, lon0) and flies along `heading` (degrees from north), at true anomaly nu0.  Velocities are the
    derivatives of the positions.  On top, a wobble A sin(W t) e / A W cos(W t) e along a fixed direction e: 4-point Hermite error
    goes as (W dt)^8, and without the wobble a node window one node off moves the root by less than float64 rounding - no test
    could see it."""
    t = np.asarray(times, LD)
    mu = LD('3.986004418e14')
    la, lo, hd = (LD(x) * PI_LD / 180 for x in (lat0, lon0, heading))
    up = np.array([np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)])
    east = np.array([-np.sin(lo), np.cos(lo), LD(0)])
    north = np.array([-np.sin(la) * np.cos(lo), -np.sin(la) * np.sin(lo), np.cos(la)])
    along = np.cos(hd) * north + np.sin(hd) * east
    nu0 = LD(nu0)
    P, Q = np.cos(nu0) * up - np.sin(nu0) * along, np.sin(nu0) * up + np.cos(nu0) * along          # towards perigee, and 90 deg on
    ecc = LD(ecc)
    n = np.sqrt(mu / LD(a) ** 3)
    E0 = 2 * np.arctan(np.sqrt((1 - ecc) / (1 + ecc)) * np.tan(nu0 / 2))
    M = E0 - ecc * np.sin(E0) + n * (t - LD(t0))
    E = M.copy()
    for _ in range(8):
        E = E - (E - ecc * np.sin(E) - M) / (1 - ecc * np.cos(E))
    b = LD(a) * np.sqrt(1 - ecc * ecc)
    x, y = LD(a) * (np.cos(E) - ecc), b * np.sin(E)
    Ed = n / (1 - ecc * np.cos(E))
    xd, yd = -LD(a) * np.sin(E) * Ed, b * np.cos(E) * Ed
    pos = x[:, None] * P + y[:, None] * Q
    vel = xd[:, None] * P + yd[:, None] * Q
    e = np.array([LD(1), LD(2), LD(3)]) / np.sqrt(LD(14))
    W = 2 * PI_LD / LD(wobble_period)
    pos = pos + (LD(wobble_m) * np.sin(W * t))[:, None] * e
    vel = vel + (LD(wobble_m) * W * np.cos(W * t))[:, None] * e
    return pos.astype(np.float64), vel.astype(np.float64)


def targets_at(st, sp, sv, t_root, look_deg, range_m):
    """float64 targets whose zero-Doppler root on the interpolated orbit is t_root (also outside the span, where the end window
    extrapolates): from the sensor there, `range_m` away at `look_deg` from the nadir (signed: either side) in the plane
    perpendicular to the velocity."""
    S, V = hermite_ld(st, sp, sv, t_root)
    unit = lambda v: v / np.sqrt((v * v).sum(-1))[:, None]
    vh = unit(V)
    up = unit(S)
    up = unit(up - (up * vh).sum(-1)[:, None] * vh)
    side = np.cross(vh, up)
    lk = np.asarray(look_deg, LD) * PI_LD / 180
    T = S + np.asarray(range_m, LD)[:, None] * (-np.cos(lk)[:, None] * up + np.sin(lk)[:, None] * side)
    return T.astype(np.float64)


def case_targets(st, sp, sv, seed, n_total=4000, n_edge=60):
    """The shuffled target set of one case: a root exactly on every node, n_edge roots each in the first and the last interval and
    0.3 to 5 s outside either end, the rest anywhere in the span; two targets with one NaN coordinate.  Returns (xyz, t_root, kind)
    with kind 0 = anywhere, 1 = node, 2 = first / last interval, 3 = outside, 4 = NaN coordinate."""
    rng = np.random.default_rng(seed)
    st = np.asarray(st, np.float64)
    n_any = n_total - st.size - 4 * n_edge
    roots = np.concatenate([st, rng.uniform(st[0], st[1], n_edge), rng.uniform(st[-2], st[-1], n_edge),
                            st[0] - rng.uniform(0.3, 5.0, n_edge), st[-1] + rng.uniform(0.3, 5.0, n_edge), rng.uniform(st[0], st[-1], n_any)])
    kind = np.concatenate([np.full(st.size, 1), np.full(2 * n_edge, 2), np.full(2 * n_edge, 3), np.zeros(n_any, int)])
    look = rng.uniform(20.0, 46.0, roots.size) * rng.choice([-1.0, 1.0], roots.size)
    xyz = targets_at(st, sp, sv, roots, look, rng.uniform(700e3, 1100e3, roots.size))
    order = rng.permutation(roots.size)                          # neighbouring lanes sit in different segments
    xyz, roots, kind = xyz[order], roots[order], kind[order]
    for k, q in enumerate(np.nonzero(kind == 0)[0][[7, -7]]):
        xyz[q, 1 + k] = np.nan
        kind[q] = 4
    return xyz, roots, kind
