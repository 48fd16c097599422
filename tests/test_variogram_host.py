"""Host side of raider_amd/variogram.py (no GPU): argument checking, PairVariogram.binned, deramp, the UTM zone choice and the fit."""
import numpy as np
import pytest

from raider_amd import variogram as V


def _pts(n=5):
    return np.arange(n, dtype=np.float64), np.zeros(n), np.ones(n)


@pytest.mark.parametrize('kw, exc, text', [
    (dict(values=np.ones((2, 2, 5))), ValueError, 'values must be'),
    (dict(x=np.arange(4.0)), ValueError, 'same length'),
    (dict(x=np.zeros(1), y=np.zeros(1), values=np.zeros(1)), ValueError, '2 .. '),
    (dict(values=np.ones((V.MAX_DATES + 1, 5))), ValueError, 'dates'),
    (dict(nbins=0), ValueError, 'nbins'),
    (dict(nbins=65), ValueError, 'nbins'),
    (dict(edges=np.linspace(0, 1, 67)), ValueError, 'at most 64 bins'),
    (dict(edges=[1.0]), ValueError, 'B >= 1'),
    (dict(edges=[0.0, 2.0, 1.0]), ValueError, 'strictly ascending'),
    (dict(edges=[0.0, 1.0, 1.0]), ValueError, 'strictly ascending'),
    (dict(edges=[0.0, np.inf]), ValueError, 'finite'),
    (dict(values=np.ones((3, 5)), edges=np.tile(np.linspace(0, 1, 4), (2, 1))), ValueError, 'one row per date'),
])
def test_pair_variogram_refuses_before_the_device(kw, exc, text):
    """every refusal comes from the Python layer: no library and no GPU context is needed to get it"""
    x, y, v = _pts()
    args = dict(x=x, y=y, values=v); args.update(kw)
    with pytest.raises(exc, match=text):
        V.pair_variogram(**args)


def test_mixed_arrays_and_tensors_are_refused():
    torch = pytest.importorskip('torch')
    x, y, v = _pts()
    with pytest.raises(TypeError, match='all NumPy arrays or all GPU tensors'):
        V.pair_variogram(torch.from_numpy(x), y, v)
    with pytest.raises(TypeError, match='on the GPU'):
        V.pair_variogram(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(v))


def test_binned_drops_empty_bins():
    count = np.array([[2, 0, 4, 0], [0, 0, 0, 0]], dtype=np.int64)
    lag = np.array([[3.0, 0.0, 10.0, 0.0], [0.0] * 4]); gam = np.array([[1.0, 0.0, 2.0, 0.0], [0.0] * 4])
    pv = V.PairVariogram(count, lag, gam, np.linspace(0, 4, 5)[None, :])
    h, g = pv.binned(0)
    assert h.tolist() == [1.5, 2.5] and g.tolist() == [0.5, 0.5]
    h, g = pv.binned(1)
    assert h.size == 0 and g.size == 0 and pv.ndates == 2


def test_default_edges_are_the_references():
    e = V.default_edges([30000.0, np.nan], 19)
    assert e.shape == (2, 20)
    assert np.array_equal(e[0], np.linspace(0, 30000.0 * 0.67, 20))       # statsPlot.py:638
    assert np.isnan(e[1][1:]).all()
    u = V._usable_rows(np.vstack([e, np.zeros((1, 20))]))
    assert np.array_equal(u[0], e[0]) and (np.diff(u[1:], axis=1) > 0).all()


def test_deramp_removes_an_exact_plane_to_roundoff():
    rng = np.random.default_rng(1)
    x = rng.uniform(3e5, 5e5, 60); y = rng.uniform(3.6e6, 3.8e6, 60)
    plane = 2.5 + 3e-6 * (x - 4e5) - 1e-6 * (y - 3.7e6)
    v = np.stack([plane, 2 * plane, plane])
    v[1, 7] = np.nan; v[2, :58] = np.nan                # a hole; a date with two valid points (no plane: returned as it is)
    out = V.deramp(x, y, v)
    assert np.nanmax(np.abs(out[:2])) <= 64 * np.finfo(float).eps * np.abs(plane).max() * 4     # round-off of a 60 x 3 solve on O(1) data
    assert np.isnan(out[1, 7]) and np.isfinite(out[1]).sum() == 59
    assert np.array_equal(out[2], v[2], equal_nan=True)
    # the reference's own three lines (:622-624) on one date
    A = np.array([x, y, np.ones(60)]).T
    noisy = plane + 0.01 * rng.standard_normal(60)
    want = noisy - np.matmul(A, np.linalg.lstsq(A, noisy.T, rcond=None)[0])
    assert np.array_equal(V.deramp(x, y, noisy), want)


@pytest.mark.parametrize('lon, lat, zone, north', [
    (-117.3, 33.9, 11, True), (-120.0, 33.9, 11, True), (-120.0000001, 33.9, 10, True), (0.0, -0.1, 31, False), (179.9, 10.0, 60, True),
    (-180.0, 10.0, 1, True), (180.0, 10.0, 1, True), (5.0, 60.0, 31, True),        # (32V would be zone 32: the exception is not reproduced)
])
def test_utm_zone_choice(lon, lat, zone, north):
    assert V.utm_zone(lon, lat) == (zone, north)


def test_fit_recovers_a_noise_free_exponential():
    """_fit_vario's default upper bound of the sill is 0.8 * max gamma, and the sill of b (1 - exp(-h / a)) lies above every sample:
    under the default bounds the truth is out of reach, in the reference as here (asserted below).  With `ub` - _fit_vario's own
    argument - opened to twice the largest sample, range and sill come back.  Least squares on noise-free data ends by xtol / ftol
    = 1e-8 (scipy's defaults, relative): 1e-6 leaves two orders for the step before the last."""
    a, b = 25000.0, 2.0
    h = np.linspace(2000.0, 120000.0, 19)
    g = V.exponential((a, b, 0.0), h)
    fit = V.fit_variogram(h, g, ub=[0.8 * h.max(), 2 * g.max(), 2 * g.max()])
    assert fit.result.success
    assert abs(fit.params[0] - a) <= 1e-6 * a and abs(fit.params[1] - b) <= 1e-6 * b
    assert fit.d_test.shape == (100,) and fit.d_test[-1] == h.max()
    clipped = V.fit_variogram(h, g)
    assert clipped.params[1] <= 0.8 * g.max() and clipped.params[1] >= 0.79 * g.max()
    with pytest.raises(ValueError):
        V.fit_variogram(h, h[:-1])
    with pytest.raises(ValueError, match='model'):
        V.fit_variogram(h, h, model='spherical')
