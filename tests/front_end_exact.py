"""The weather-model front end (csrc/producer_kernels.h) restated as references that share no code with the oracle - the yardstick of
tests/test_front_end_exact_host.py (no GPU) and tests/test_gpu_front_end_edges.py.  Not a test module.

    producer_exact(zs, p, t, hum, kind, new_z, zmin)     models/weatherModel.py:235-262 per column, in plain loops
    ztd_exact(pointwise_f32, out_z) / ztd_ratio(...)     the suffix trapezoid sums of _getZTD in long double (or exact rationals)
    ecmwf_levels_exact(z_surf, lnsp, t, q, lats, a, b)   utilFcns.calcgeoh + geo_to_ht with 40 digits
    geo_to_ht_exact(lat, gh)                             utilFcns.geo_to_ht with 40 digits
    hybrid_cases() / measure_k64()                       the two hybrid-level states of the tests, and what float64 / float32 NumPy
                                                         evaluations of calcgeoh lose on them

What is exact and what is IEEE.  The producer has ONE transcendental step: the saturation vapour pressure (find_svp, weatherModel.py
:750-780).  It is evaluated here with mpmath (40 digits) on the double constants of the formula and rounded ONCE to float32, which is
what the reference's `(svp * 100).astype(float32)` gives unless the exact value lies within the float64 evaluation's own error of a
float32 rounding tie: the distance to the nearest tie is returned with it, in float64 ulps, and values closer than TIE_ULPS are
flagged, together with everything computed from them.  Every later step is +, -, *, / and casts in an order the reference fixes,
restated with Python floats (IEEE doubles) and np.float32 scalars: these are reproducible to the bit, on any platform.

The hybrid levels are ill-conditioned (dlogP is a difference of logarithms, alpha = 1 - P0 / (P1 - P0) dlogP cancels), so the exact
value comes with a condition sum per level, C = (sum |TRd dlogP| over the levels below + |TRd alpha| + |z_surf|) / g0 [m]: the scale on
which a float64 evaluation may be held, `k eps C`.
"""
import fractions
import functools
import math
from pathlib import Path

import mpmath as mp
import numpy as np

DPS = 40
LD = np.longdouble
F32 = np.float32
EPS = 2.0 ** -52
TIE_ULPS = 4.0
HAVE_LD = np.finfo(LD).nmant >= 63
_NAN32 = F32(np.nan)


# ---- find_svp ---------------------------------------------------------------------------------------------------------------------
def _round_once_f32(v):
    """mpf v > 0 -> (nearest float32, |v - nearest rounding tie| in float64 ulps of v)"""
    f = F32(float(v))
    for _ in range(2):                                  # (float(v) rounds to double first: step to the neighbour if that crossed a tie)
        up, dn = np.nextafter(f, F32(np.inf)), np.nextafter(f, F32(-np.inf))
        hi, lo = (mp.mpf(float(f)) + mp.mpf(float(up))) / 2, (mp.mpf(float(f)) + mp.mpf(float(dn))) / 2
        if v > hi:
            f = up
        elif v < lo:
            f = dn
        else:
            break
    ulp64 = math.ldexp(1.0, math.frexp(float(v))[1] - 53)
    return f, float(min(abs(v - lo), abs(v - hi)) / ulp64)


@functools.lru_cache(maxsize=None)
def svp_exact(t):
    """find_svp at one temperature (a Python float): (svp in Pa as float32, distance to the nearest float32 tie in float64 ulps)"""
    if t != t:
        return _NAN32, math.inf
    with mp.workdps(DPS):
        T, t1, t2, c = mp.mpf(t), mp.mpf(273.15), mp.mpf(250.15), mp.mpf(6.1121)
        tref = T - t1
        water = lambda: c * mp.exp((mp.mpf(17.502) * tref) / (mp.mpf(240.97) + tref))
        ice = lambda: c * mp.exp((mp.mpf(22.587) * tref) / (mp.mpf(273.86) + tref))
        if t > 273.15:
            v = water()
        elif t < 250.15:
            v = ice()
        else:
            wgt = (T - t2) / (t1 - t2)
            i = ice()
            v = i + (water() - i) * wgt ** 2
        return _round_once_f32(v * 100)


# ---- the producer -----------------------------------------------------------------------------------------------------------------
def _upper(xs, x):
    """interpolate.h:23-38 bisect_left: the first index with x < xs[i]"""
    left, right = 0, len(xs)
    while right != left:
        mid = (left + right) // 2
        if x < xs[mid]:
            right = mid
        else:
            left = mid + 1
    return right


def _resample(xs, ys, dirty, new_z):
    """interpolate_1d (interpolate.h:78-118) with fill NaN, cast to float32: (values, depends-on-a-flagged-svp)"""
    n = len(xs)
    out, od = [], []
    for x in new_z:
        hi = _upper(xs, x)
        if hi < 1 or hi > n - 1:
            out.append(_NAN32); od.append(False)
            continue
        x0, x1, y0, y1 = xs[hi - 1], xs[hi], ys[hi - 1], ys[hi]
        slope = (y1 - y0) / (x1 - x0)
        out.append(F32(y0 + slope * (x - x0)))
        od.append(dirty[hi - 1] or dirty[hi])
    return out, od


def _fill(col, fill, dirty):
    """interpolator.fillna3D (:110-130) on one column of float32: leading NaNs <- the first valid value, interior runs linear in the
    INDEX (np.interp on float64: slope (j - i) + a, cast back), trailing NaNs <- fill"""
    n = len(col)
    valid = [j for j in range(n) if col[j] == col[j]]
    if not valid:
        return [F32(fill)] * n, [False] * n
    first, last = valid[0], valid[-1]
    out, od = list(col), list(dirty)
    for j in range(n):
        if col[j] == col[j]:
            continue
        if j > last:
            out[j], od[j] = F32(fill), False
        elif j < first:
            out[j], od[j] = col[first], dirty[first]
        else:
            i = j - 1
            while col[i] != col[i]:
                i -= 1
            k = j + 1
            while col[k] != col[k]:
                k += 1
            a, b = float(col[i]), float(col[k])
            slope = (b - a) / float(k - i)
            out[j], od[j] = F32(slope * float(j - i) + a), dirty[i] or dirty[k]
    return out, od


def producer_exact(zs, p, t, hum, kind, new_z, zmin=-100.0, k1=0.776, k2=0.233, k3=3.75e3, R_v=461.524, R_d=287.06):
    """models/weatherModel.py:235-262 on (..., nlev) columns with ascending heights.  Returns a dict: zs (the output heights, with the
    pad level when zmin lies below them), t, p, e, wet, hydro (float32, (..., nzo)), t_u, p_u, e_u (the resampled state BEFORE the fill,
    (..., nz)), flagged ((..., nzo) bool: e and wet there depend on an svp within TIE_ULPS of a float32 tie), svp_tie ((..., nlev) the
    distances in float64 ulps)."""
    if kind not in ('q', 'rh'):
        raise RuntimeError('Not a valid humidity type')
    zs, p, t, hum = (np.asarray(v, dtype=np.float64) for v in (zs, p, t, hum))
    lead, nlev = zs.shape[:-1], zs.shape[-1]
    new_z = [float(v) for v in np.asarray(new_z, dtype=np.float64)]
    pad = float(zmin) < min(new_z)
    nz, nzo = len(new_z), len(new_z) + (1 if pad else 0)
    ncol = int(np.prod(lead, dtype=np.int64))
    Z, P, T, H = (v.reshape(ncol, nlev).tolist() for v in (zs, p, t, hum))
    fk1, fk2, fk3 = F32(k1), F32(k2), F32(k3)
    names = ('t', 'p', 'e', 'wet', 'hydro')
    out = {k: np.empty((ncol, nzo), np.float32) for k in names}
    raw = {k: np.empty((ncol, nz), np.float32) for k in ('t_u', 'p_u', 'e_u')}
    flagged = np.zeros((ncol, nzo), bool)
    tie = np.empty((ncol, nlev))
    for c in range(ncol):
        e, dirty = [], []
        for l in range(nlev):
            svp32, dist = svp_exact(T[c][l])
            tie[c, l] = dist
            s = float(svp32)
            if kind == 'q':
                w = H[c][l] / (1.0 - H[c][l])
                e.append(w * R_v * (P[c][l] - s) / R_d)                           # weatherModel.py:348
            else:
                e.append(H[c][l] / 100.0 * s)                                       # :353
            dirty.append(dist < TIE_ULPS)
        clean = [False] * nlev
        tu, _ = _resample(Z[c], T[c], clean, new_z)
        pu, _ = _resample(Z[c], P[c], clean, new_z)
        eu, du = _resample(Z[c], e, dirty, new_z)
        raw['t_u'][c], raw['p_u'][c], raw['e_u'][c] = tu, pu, eu
        pf, _ = _fill(pu, 0.0, [False] * nz)
        tf, _ = _fill(tu, 1e16, [False] * nz)
        ef, df = _fill(eu, 0.0, du)
        wet = [(fk2 * ef[j]) / tf[j] + (fk3 * ef[j]) / (tf[j] * tf[j]) for j in range(nz)]      # :357, float32 arithmetic
        hyd = [(fk1 * pf[j]) / tf[j] for j in range(nz)]                                        # :361
        cols = dict(t=tf, p=pf, e=ef, wet=wet, hydro=hyd)
        for k in names:
            out[k][c] = ([cols[k][0]] if pad else []) + cols[k]                                 # utilFcns.padLower
        flagged[c] = ([df[0]] if pad else []) + df
    res = {k: v.reshape(lead + (nzo,)) for k, v in out.items()}
    res.update({k: v.reshape(lead + (nz,)) for k, v in raw.items()})
    res['zs'] = np.array(([float(zmin)] if pad else []) + new_z)
    res['flagged'] = flagged.reshape(lead + (nzo,))
    res['svp_tie'] = tie.reshape(lead + (nlev,))
    return res


# ---- _getZTD ----------------------------------------------------------------------------------------------------------------------
def ztd_exact(pointwise_f32, out_z):
    """weatherModel.py:389-403 on a (..., nzo) float32 field: S[j] = 1e-6 sum_{k >= j} d_k (f[k+1] + f[k]) / 2 and A[j] = 1e-6 sum_{k >= j}
    |d_k (f[k+1] + f[k]) / 2|.  f[k+1] + f[k] is the float32 sum np.trapz forms (an IEEE step, reproduced); the differences of the
    heights, the products and the sums are long double, whose own error (two roundings per term, nzo additions: <= (nzo + 2) 2^-64 A,
    0.13 eps64 A at 512 levels) is far inside any bound stated in eps64 A - or exact rationals where long double has no 64-bit mantissa.
    1e-6 is the double nearest to it, as in the reference.  Returns (S, A): long double arrays, or object arrays of Fractions."""
    f = np.asarray(pointwise_f32)
    assert f.dtype == np.float32
    z = np.asarray(out_z, dtype=np.float64)
    s32 = f[..., 1:] + f[..., :-1]
    assert s32.dtype == np.float32
    zero = np.zeros(f.shape[:-1] + (1,))
    if HAVE_LD:
        term = (z[1:].astype(LD) - z[:-1].astype(LD)) * s32.astype(LD) / LD(2)
        suffix = lambda v: np.concatenate([np.cumsum(v[..., ::-1], axis=-1)[..., ::-1], zero.astype(LD)], axis=-1)
        return LD(1e-6) * suffix(term), LD(1e-6) * suffix(np.abs(term))
    F = fractions.Fraction
    d = [F(float(b)) - F(float(a)) for a, b in zip(z[:-1], z[1:])]
    S, A = np.empty(f.shape, object), np.empty(f.shape, object)
    flat_s, flat_S, flat_A = s32.reshape(-1, s32.shape[-1]), S.reshape(-1, f.shape[-1]), A.reshape(-1, f.shape[-1])
    for c in range(flat_s.shape[0]):
        acc = acc_abs = F(0)
        flat_S[c, -1] = flat_A[c, -1] = F(0)
        for k in range(len(d) - 1, -1, -1):
            term = d[k] * F(float(flat_s[c, k])) / 2
            acc += term; acc_abs += abs(term)
            flat_S[c, k], flat_A[c, k] = F(1e-6) * acc, F(1e-6) * acc_abs
    return S, A


def ztd_ratio(total, S, A):
    """|total - S| / (eps64 A) per element as float64 (0 where both the difference and A vanish, inf where only A does)"""
    total = np.asarray(total, dtype=np.float64)
    if HAVE_LD:
        d, lim = np.abs(total.astype(LD) - S), LD(EPS) * A
    else:
        F = fractions.Fraction
        d = np.frompyfunc(lambda g, s: abs(F(float(g)) - s), 2, 1)(total, S)
        lim = np.frompyfunc(lambda a: F(EPS) * a, 1, 1)(A)
    out = np.zeros(total.shape)
    pos = np.asarray(lim > 0, dtype=bool)
    out[pos] = np.asarray(d[pos] / lim[pos], dtype=np.float64)
    out[~pos & np.asarray(d != 0, dtype=bool)] = np.inf
    return out


# ---- hybrid model levels ----------------------------------------------------------------------------------------------------------
def _geo_constants(lat_deg):
    """_get_g_ll (utilFcns.py:351-353) and get_Re (:356-375) at one latitude [deg, taken as the exact double]: (g_ll / g0, Re) as mpf"""
    lat = mp.radians(mp.mpf(float(lat_deg)))
    c2 = mp.cos(2 * lat)
    g_ll = mp.mpf(9.80616) * (1 - mp.mpf(0.002637) * c2 + mp.mpf(0.0000059) * c2 ** 2)
    re = mp.sqrt(1 / (mp.cos(lat) ** 2 / mp.mpf(6378137.0) ** 2 + mp.sin(lat) ** 2 / mp.mpf(6356752.0) ** 2))
    return g_ll / mp.mpf(9.80665), re


def geo_to_ht_exact(lats, gh):
    """utilFcns.geo_to_ht (:378-410) with 40 digits: lats broadcast against the leading axes of gh (..., n) -> float64 heights"""
    gh = np.asarray(gh, dtype=np.float64)
    lats = np.broadcast_to(np.asarray(lats, dtype=np.float64), gh.shape[:-1])
    out = np.empty(gh.shape)
    with mp.workdps(DPS):
        for idx in np.ndindex(*gh.shape[:-1]):
            g, re = _geo_constants(lats[idx])
            gre = g * re
            out[idx] = [float((mp.mpf(float(v)) * re) / (gre - mp.mpf(float(v)))) for v in gh[idx]]
    return out


def ecmwf_levels_exact(z_surf, lnsp, t, q, lats, a, b, R_d=287.06):
    """utilFcns.calcgeoh (:781-859) + geo_to_ht on the float32 inputs, every constant the double the formulas name, 40 digits; the
    re-ordering of ecmwf.py:92-110.  t, q: (nlev, ny, nx), level 1 = model top.  Returns (p, zs, C), each (ny, nx, nlev) float64 with the
    bottom level first: pressure and height rounded once to double, and the condition sum C [m] of the module docstring.  A column
    whose lnsp is NaN is NaN."""
    z_surf, lnsp, t, q, lats = (np.asarray(v, dtype=np.float32) for v in (z_surf, lnsp, t, q, lats))
    nlev, ny, nx = t.shape
    p, zs, C = (np.full((ny, nx, nlev), np.nan) for _ in range(3))
    with mp.workdps(DPS):
        g0, Rd = mp.mpf(9.80665), mp.mpf(float(R_d))
        am, bm = [mp.mpf(float(v)) for v in a], [mp.mpf(float(v)) for v in b]
        assert len(am) == nlev + 1 and len(bm) == nlev + 1
        for iy in range(ny):
            g, re = _geo_constants(lats[iy])
            gre = g * re
            for ix in range(nx):
                if lnsp[iy, ix] != lnsp[iy, ix]:
                    continue
                sp, z0 = mp.exp(mp.mpf(float(lnsp[iy, ix]))), mp.mpf(float(z_surf[iy, ix]))
                z_h = below = mp.mpf(0)
                for lev in range(nlev, 0, -1):
                    tl = mp.mpf(float(t[lev - 1, iy, ix])) * (1 + mp.mpf(0.609133) * mp.mpf(float(q[lev - 1, iy, ix])))
                    ph, ph1 = am[lev - 1] + bm[lev - 1] * sp, am[lev] + bm[lev] * sp
                    if lev == 1:
                        dlogp, alpha = mp.log(ph1 / mp.mpf(0.1)), mp.log(2)
                    else:
                        dlogp = mp.log(ph1 / ph)
                        alpha = 1 - (ph / (ph1 - ph)) * dlogp
                    trd = tl * Rd
                    gh = (z_h + trd * alpha + z0) / g0
                    o = nlev - lev
                    p[iy, ix, o] = float(ph)
                    zs[iy, ix, o] = float((gh * re) / (gre - gh))
                    C[iy, ix, o] = float((below + abs(trd * alpha) + abs(z0)) / g0)
                    z_h += trd * dlogp
                    below += abs(trd * dlogp)
    return p, zs, C


# ---- the two hybrid-level states of the tests, and what NumPy loses on them --------------------------------------------------------
RAW_FILE = Path(__file__).resolve().parent / 'golden' / 'ref_files' / 'ERA-5_2019_11_17_T20_51_58.nc'
A8 = np.array([0.0, 2000.0, 6000.0, 11000.0, 13000.0, 9000.0, 4000.0, 1000.0, 0.0])
B8 = np.array([0.0, 0.0, 0.02, 0.1, 0.3, 0.55, 0.8, 0.95, 1.0])


def synthetic_hybrid_state():
    """8 levels on the table (A8, B8); 7 rows at latitudes -90 .. 0 .. 90 by 5 columns; surface pressures 50 .. 108 kPa; surfaces from
    420 m below sea level to 5.5 km; one column (row 2, column 3) without a surface pressure"""
    rng = np.random.default_rng(8)
    ny, nx, nlev = 7, 5, 8
    lats = np.array([-90.0, -60.5, -33.25, 0.0, 21.125, 47.5, 90.0], np.float32)
    sp = np.linspace(50000.0, 108000.0, ny * nx).reshape(ny, nx)
    sp = sp[:, rng.permutation(nx)]
    lnsp = np.log(sp).astype(np.float32)
    z_surf = (9.80665 * (5500.0 * (108000.0 - sp) / 58000.0 - 420.0 * (sp > 100000.0))).astype(np.float32)
    frac = (np.arange(nlev) + 0.5)[:, None, None] / nlev                       # level 1 = top
    t = (215.0 + 75.0 * frac ** 1.5 + rng.normal(0, 1.5, (nlev, ny, nx))).astype(np.float32)
    q = (0.012 * frac ** 3 * rng.uniform(0.5, 1.5, (nlev, ny, nx))).astype(np.float32)
    lnsp[2, 3] = np.nan
    return dict(z=z_surf, lnsp=lnsp, t=t, q=q, lats=lats, a=A8, b=B8)


@functools.lru_cache(maxsize=None)
def hybrid_cases():
    """{name: (state, (p, zs, C) exact)}: a 6 x 6 block of the reference's raw ERA-5 model-level file on all 137 levels, and the
    synthetic state"""
    from oracle import raider_oracle as O
    tab = np.load(Path(__file__).resolve().parent.parent / 'raider_amd' / 'data' / 'ecmwf_l137.npz')
    r = O.read_ecmwf_model_level_file(RAW_FILE)
    c = np.ascontiguousarray
    block = dict(z=c(r['z'][2:8, 3:9]), lnsp=c(r['lnsp'][2:8, 3:9]), t=c(r['t'][:, 2:8, 3:9]), q=c(r['q'][:, 2:8, 3:9]), lats=c(r['lats'][2:8]),
                 a=tab['a'], b=tab['b'])
    assert block['t'].shape == (137, 6, 6)
    out = {}
    for name, s in (('block', block), ('synthetic', synthetic_hybrid_state())):
        out[name] = (s, ecmwf_levels_exact(s['z'], s['lnsp'], s['t'], s['q'], s['lats'], s['a'], s['b']))
    return out


@functools.lru_cache(maxsize=None)
def measure_k64():
    """The oracle's NumPy evaluations of calcgeoh + geo_to_ht against the exact heights on hybrid_cases(): {name: (k64, d32)} with
    k64 = max |float64 evaluation - exact| / (eps64 C) and d32 = max |float32 evaluation - exact| in metres, and 'k64' / 'd32': the
    worst of each."""
    from oracle import raider_oracle as O
    out = {}
    for name, (s, (p, zs, C)) in hybrid_cases().items():
        ok = np.isfinite(zs)
        args = (s['z'], s['lnsp'], s['t'], s['q'], s['lats'], s['a'], s['b'])
        _, h64 = O.ecmwf_model_levels(*args, dtype=np.float64)
        _, h32 = O.ecmwf_model_levels(*args, dtype=np.float32)
        assert np.array_equal(np.isfinite(h64), ok)
        out[name] = (float(np.max(np.abs(h64 - zs)[ok] / (EPS * C[ok]))), float(np.max(np.abs(h32.astype(np.float64) - zs)[ok])))
    out['k64'] = max(v[0] for v in out.values())
    out['d32'] = max(v[1] for k, v in out.items() if k != 'k64')
    return out
