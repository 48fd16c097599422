"""The references of tests/front_end_exact.py pinned without a GPU: producer_exact on golden g10 (made by the reference's own WeatherModel)
and on the oracle's missing-data scene; ecmwf_levels_exact against the oracle's float64 and float32 NumPy evaluations of calcgeoh +
geo_to_ht - which measures what DESIGN.md 6.5 states: k64, the float64 evaluation's distance to the exact heights in units of
eps C, and the float32 evaluation's distance in metres."""
import numpy as np
import pytest

from oracle import raider_oracle as O
from tests import front_end_exact as X                    # (imports mpmath: its absence is an error here, not a skip)


@pytest.mark.parametrize('tag', ['q', 'rh'])
def test_producer_exact_equals_reference_golden(golden, tag):
    """t, p, hydro, the unfilled state and its NaN pattern bit for bit; e and wet bit for bit wherever no svp behind them lies within
    4 float64 ulps of a float32 rounding tie (there the reference's float64 exp may have rounded either way)."""
    g = golden('g10_cube_producer')
    r = X.producer_exact(g[f'{tag}_zs'], g[f'{tag}_p'], g[f'{tag}_t'], g[f'{tag}_hum'], tag, g[f'{tag}_newz'])
    assert np.array_equal(r['zs'], g[f'{tag}_out_zs'])
    for k in ('t', 'p'):
        assert np.array_equal(r[f'{k}_u'], g[f'{tag}_{k}_u'], equal_nan=True), k
        assert np.array_equal(r[k], g[f'{tag}_{k}_out']), k
    assert np.isnan(r['t_u']).any() and np.array_equal(np.isnan(r['e_u']), np.isnan(g[f'{tag}_e_u']))
    assert np.array_equal(r['hydro'], g[f'{tag}_hydro'])
    near = r['svp_tie'] < X.TIE_ULPS
    print(f'g10 {tag}: {int(near.sum())} of {near.size} svp values within {X.TIE_ULPS:g} float64 ulps of a float32 tie (closest {r["svp_tie"].min():.3g}), '
          f'{int(r["flagged"].sum())} output values flagged')
    keep = ~r['flagged']
    assert keep.mean() > 0.99
    assert np.array_equal(r['e'][keep], g[f'{tag}_e_out'][keep])
    assert np.array_equal(r['wet'][keep], g[f'{tag}_wet'][keep])
    for name in ('wet', 'hydro'):                                   # and the golden's own totals sit on the exact sums of its point-wise fields
        S, A = X.ztd_exact(g[f'{tag}_{name}'], g[f'{tag}_out_zs'])
        ratio = X.ztd_ratio(g[f'{tag}_{name}_total'], S, A)
        assert ratio.max() <= 2 + g[f'{tag}_out_zs'].size + 1, ratio.max()          # two roundings per term, n additions, the scale
        assert np.all(g[f'{tag}_{name}_total'][..., -1] == 0.0)


def missing_data_scene():
    """the scene of tests/test_gpu_producer.py::test_producer_vs_oracle_with_missing_data"""
    rng = np.random.default_rng(77)
    A, B, nl = 9, 11, 37
    base = np.sort(rng.uniform(0, 1, (A, B, nl)), axis=2)
    zs = -80.0 + 300.0 * rng.uniform(0, 1, (A, B, 1)) + 42000.0 * base ** 1.4
    t = np.maximum(289.0 - 0.0063 * zs + rng.normal(0, 0.4, zs.shape), 203.0)
    p = 101000.0 * np.exp(-zs / 7700.0)
    q = 0.011 * np.exp(-zs / 2500.0)
    t[1, 2, 10:14] = np.nan
    t[3, 3, :] = np.nan
    p[4, 5, 20:] = np.nan
    newz = np.concatenate([np.arange(-100.0, 3000.0, 150.0), np.arange(3000.0, 44000.0, 1500.0)])
    return zs, p, t, q, newz


def test_producer_exact_agrees_with_oracle_on_missing_data():
    zs, p, t, q, newz = missing_data_scene()
    want = O.cube_from_model_levels(zs, p, t, q, 'q', newz)
    r = X.producer_exact(zs, p, t, q, 'q', newz)
    assert np.array_equal(r['zs'], want['zs'])
    for k in ('t_u', 'p_u'):
        assert np.array_equal(r[k], want[k], equal_nan=True), k
    assert np.array_equal(np.isnan(r['e_u']), np.isnan(want['e_u']))
    for k in ('t', 'p', 'hydro'):
        assert np.array_equal(r[k], want[k]), k
    keep = ~r['flagged']
    assert keep.mean() > 0.99
    assert np.array_equal(r['e'][keep], want['e'][keep]) and np.array_equal(r['wet'][keep], want['wet'][keep])


def test_svp_exact_at_the_branch_temperatures():
    """250.15 K and 273.15 K belong to the blend (weights exactly 0 and 1: pure ice, pure water = 611.21 Pa), one ulp outside to the pure
    branches; the oracle's float64 evaluation rounds to the same float32 everywhere here"""
    assert X.svp_exact(273.15)[0] == np.float32(611.21)
    for base in (250.15, 273.15):
        for t in (np.nextafter(base, 0.0), base, np.nextafter(base, 1e3)):
            got, dist = X.svp_exact(float(t))
            assert dist >= X.TIE_ULPS and got == O.find_svp(np.array([t]))[0], (t, got, dist)


def test_ztd_exact_on_a_column_with_known_sums():
    """powers of two: every term and sum is exact, in any precision"""
    z = np.array([-64.0, 0.0, 32.0, 160.0])
    f = np.array([[4.0, 2.0, 1.0, 0.5], [-4.0, 2.0, -1.0, 0.5]], np.float32)
    S, A = X.ztd_exact(f, z)
    want = np.array([[192.0 + 48.0 + 96.0, 48.0 + 96.0, 96.0, 0.0], [-64.0 + 16.0 - 32.0, 16.0 - 32.0, -32.0, 0.0]])
    want_abs = np.array([[336.0, 144.0, 96.0, 0.0], [112.0, 48.0, 32.0, 0.0]])
    assert np.all(X.ztd_ratio(1e-6 * want, S, A) <= 1.0)              # (1e-6 x is one rounding)
    assert np.all(X.ztd_ratio(1e-6 * want_abs, A, A) <= 1.0)
    assert np.isinf(X.ztd_ratio(np.full((2, 4), 1.0), S, A)[:, -1]).all()


def test_hybrid_levels_float64_and_float32_against_exact():
    """DESIGN.md 6.5 measured: the float64 evaluation sits k64 eps C from the exact heights, the float32 one (what the reference ran)
    metres away"""
    m = X.measure_k64()
    for name, (s, (p, zs, C)) in X.hybrid_cases().items():
        ok = np.isfinite(zs)
        p64, _ = O.ecmwf_model_levels(s['z'], s['lnsp'], s['t'], s['q'], s['lats'], s['a'], s['b'], dtype=np.float64)
        assert np.array_equal(np.isnan(p64), ~ok) and (~ok).sum() == (0 if name == 'block' else s['t'].shape[0])
        assert np.all(np.abs(p64 - p)[ok] <= np.spacing(np.abs(p[ok])))
        assert np.all(np.diff(zs, axis=2)[ok[..., 1:]] > 0) and np.all(C[ok] > 0)
        print(f'hybrid levels, {name} {s["t"].shape}: k64 = {m[name][0]:.4g} (|float64 - exact| / (eps C)), |float32 - exact| up to {m[name][1]:.4g} m; '
              f'C from {C[ok].min():.4g} to {C[ok].max():.4g} m')
    print(f'hybrid levels: k64 = {m["k64"]:.4g}, float32 distance = {m["d32"]:.4g} m')
    assert np.isfinite(m['k64']) and m['k64'] > 0
    assert m['d32'] > 0.5


def test_geo_to_ht_exact_against_the_known_radii():
    """get_Re's doctest values (utilFcns.py:366-373): a zero geopotential height maps to 0, and h (g_ll / g0 Re - gh) = gh Re"""
    lats = np.array([0.0, 30.0, 45.0, 60.0, 90.0])
    h = X.geo_to_ht_exact(lats, np.array([[0.0, 1000.0, 60000.0]] * 5))
    assert np.all(h[:, 0] == 0.0)
    re = np.array([6378137.0, 6372770.5219805, 6367417.56705189, 6362078.07851428, 6356752.0])
    g_ll = 9.80616 * (1 - 0.002637 * np.cos(np.radians(2 * lats)) + 0.0000059 * np.cos(np.radians(2 * lats)) ** 2)
    np.testing.assert_allclose(h[:, 1:] * (g_ll / 9.80665 * re)[:, None] - h[:, 1:] * np.array([1000.0, 60000.0]), np.array([1000.0, 60000.0]) * re[:, None],
                               rtol=1e-13)
