"""GPU: exact all-pair variograms (rdr_pair_distance_max / rdr_pair_variogram, csrc/variogram_kernels.h; raider_amd/variogram.py).

Yardstick: a NumPy all-pairs restatement inside this file - triu_indices, np.sqrt(dx*dx + dy*dy), the bin masks of
cli/statsPlot.py:644 and math.fsum per bin.

Conditions, none of them tuned on the device's results:
  * COUNTS ARE EXACT.  Coordinates lie on an integer-metre lattice and edges are chosen off it; before a device result is looked at,
    NumPy alone asserts that no pair's h lies within a relative 1e-12 of any edge (for an edge that is exactly 0 the comparison
    h <= 0 is exact in any arithmetic - h = sqrt(0) = 0 for coincident stations - and needs no margin).  For the default edges the
    same is asserted against edges made from NumPy's own hmax.
  * hmax is within 2 ulp of NumPy's: contraction could move d^2 by at most 1 ulp and the square root rounds once more.  The kernels
    are compiled with contraction off for d^2 and the largest |difference| seen is printed: 0 ulp in every case when this was written.
  * lag_sum and gamma_sum per bin are within a relative (m + 4) * 2^-52 of the fsum value, m the bin's count: the bound for m
    non-negative f64 terms added in any order, (m - 1) * 2^-53 to first order, plus the terms' own roundings.  An empty bin is exactly 0.

Shapes: N = 2, 3 (the smallest), 63 / 64 / 65 (one wave and one more), TILE, TILE + 1, 2 TILE + 17 (diagonal and off-diagonal tiles,
a ragged last tile), 1500 once (21 tile pairs); D = 1, 4, 5, 9 (one group, a full group, groups with a remainder: 4 + 1, 4 + 4 + 1) and
2, 3 (the group of two); B = 1, 19, 64; one shared edge row and one per date; float32 values; a station that is NaN on some dates, a
date that is all NaN, a date with one valid point; two stations at one place; host arrays, device pointers and tensors.
"""
import ctypes as C
import functools
import math
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import raider_amd as R                                     # noqa: E402
from raider_amd import _lib as L                           # noqa: E402
from raider_amd import variogram as V                      # noqa: E402

T = V.TILE
GOLDEN = Path(__file__).resolve().parent / 'golden' / 'g20_variogram.npz'


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------
def pair_lags(x, y):
    i, j = np.triu_indices(x.size, 1)
    dx = x[i] - x[j]; dy = y[i] - y[j]
    return i, j, np.sqrt(dx * dx + dy * dy)


def numpy_hmax(x, y, v):
    i, j, h = pair_lags(x, y)
    out = np.full(v.shape[0], np.nan)
    for d in range(v.shape[0]):
        ok = ~np.isnan(v[d][i]) & ~np.isnan(v[d][j])
        if ok.any():
            out[d] = h[ok].max()
    return out


def numpy_variogram(x, y, v, edges):
    """count, lag_sum, gamma_sum [D, B] of float64 values v [D, N] by the masks of statsPlot.py:644 and math.fsum"""
    i, j, h = pair_lags(x, y)
    D, B = v.shape[0], edges.shape[1] - 1
    count = np.zeros((D, B), dtype=np.int64); lag = np.zeros((D, B)); gam = np.zeros((D, B))
    for d in range(D):
        e = edges[d if edges.shape[0] > 1 else 0]
        ok = ~np.isnan(v[d][i]) & ~np.isnan(v[d][j])
        hd = h[ok]
        g = 0.5 * np.square(v[d][i][ok] - v[d][j][ok])
        for b in range(B):
            m = np.logical_and(e[b] < hd, hd <= e[b + 1])
            count[d, b] = m.sum(); lag[d, b] = math.fsum(hd[m]); gam[d, b] = math.fsum(g[m])
    return count, lag, gam


def assert_off_edges(x, y, edges):
    """the condition on the INPUTS that makes counts exact: no h within a relative 1e-12 of an edge (an edge of exactly 0 aside)"""
    _, _, h = pair_lags(x, y)
    for e in np.unique(edges[np.isfinite(edges)]):
        if e != 0.0:
            assert np.abs(h - e).min() > 1e-12 * abs(e), f'the test inputs put a pair on the edge {e!r}'


def assert_sums(got_count, got_lag, got_gam, want):
    count, lag, gam = want
    assert got_count.dtype == np.int64 and np.array_equal(got_count, count)
    tol = (count + 4) * 2.0 ** -52
    for got, ref, name in ((got_lag, lag, 'lag_sum'), (got_gam, gam, 'gamma_sum')):
        assert np.all(got[count == 0] == 0.0), name
        err = np.abs(got - ref)
        assert np.all(err <= tol * np.abs(ref)), (name, (err / np.maximum(np.abs(ref), 1e-300) / 2.0 ** -52).max(), count.max())


# ---- cases -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(n, d=1, b=19, per_date=False, f32=False, holes=False, dup=False, seed=0):
    """inputs and the NumPy result, computed once and shared by the routes (arrays are never written to)"""
    rng = np.random.default_rng(1000 * n + 10 * d + seed)
    nodes = rng.choice(6000 * 4000, size=n, replace=False)          # distinct nodes of an integer-metre lattice: h^2 is an integer
    x = (nodes % 6000).astype(np.float64) + 412000.0
    y = (nodes // 6000).astype(np.float64) + 3765000.0
    if dup and n >= 3:
        x[n - 1], y[n - 1] = x[0], y[0]                             # two stations at one place
    v = 2.4 + 0.05 * rng.standard_normal((d, n))
    if f32:
        v = v.astype(np.float32)
    if holes:
        v[::2, min(1, n - 1)] = np.nan                              # a station missing on every other date
        if d >= 2:
            v[1, :] = np.nan                                        # a date without data
        if d >= 3:
            v[2, :] = np.nan; v[2, n // 2] = 1.0                    # a date with one valid point
    v64 = v.astype(np.float64)
    _, _, h = pair_lags(x, y)
    top = h.max()
    rows = d if per_date else 1
    edges = np.stack([np.linspace(0.37 + 3.1 * r, (0.67 - 0.03 * r) * top + 0.113, b + 1) for r in range(rows)])
    assert_off_edges(x, y, edges)
    for a in (x, y, v, edges):
        a.setflags(write=False)
    return dict(x=x, y=y, v=v, v64=v64, edges=edges, want=numpy_variogram(x, y, v64, edges), hmax=numpy_hmax(x, y, v64))


SHAPES = [dict(n=2), dict(n=3), dict(n=63), dict(n=64), dict(n=65), dict(n=T), dict(n=T + 1), dict(n=2 * T + 17),
          dict(n=65, d=4), dict(n=T + 1, d=5, per_date=True), dict(n=65, d=9, holes=True), dict(n=65, d=2), dict(n=64, d=3, per_date=True, holes=True),
          dict(n=65, b=1), dict(n=T + 1, b=64), dict(n=65, d=5, b=64, per_date=True, holes=True),
          dict(n=65, d=4, f32=True), dict(n=T + 1, d=3, holes=True, dup=True), dict(n=3, dup=True), dict(n=2, d=3, holes=True)]
IDS = ['-'.join(f'{k}{v if not isinstance(v, bool) else ""}' for k, v in s.items()) for s in SHAPES]


def call_host(c, edges=None, nbins=19):
    return V.pair_variogram(c['x'], c['y'], c['v'], edges=c['edges'] if edges is None else edges, nbins=nbins)


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_host_route_against_numpy(shape):
    c = case(**shape)
    pv = call_host(c)
    assert isinstance(pv.count, np.ndarray) and pv.hmax is None
    assert_sums(pv.count, pv.lag_sum, pv.gamma_sum, c['want'])


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_tensor_route_against_numpy(shape):
    """tensors in, tensors out - the same counts, byte for byte, as the host route's yardstick; float32 tensors are widened on the device"""
    import torch
    c = case(**shape)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    pv = V.pair_variogram(dev(c['x']), dev(c['y']), dev(c['v']), edges=dev(c['edges']))
    for t in (pv.count, pv.lag_sum, pv.gamma_sum, pv.edges):
        assert torch.is_tensor(t) and t.is_cuda
    assert pv.count.dtype == torch.int64 and pv.lag_sum.dtype == torch.float64
    assert_sums(pv.count.cpu().numpy(), pv.lag_sum.cpu().numpy(), pv.gamma_sum.cpu().numpy(), c['want'])
    h, g = pv.binned(0)
    assert torch.is_tensor(h) and h.numel() == int((c['want'][0][0] > 0).sum())


@pytest.mark.parametrize('shape', [dict(n=2), dict(n=65, d=9, holes=True), dict(n=2 * T + 17), dict(n=T + 1, d=3, holes=True, dup=True), dict(n=2, d=3, holes=True)],
                         ids=lambda s: '-'.join(f'{k}{v}' for k, v in s.items()))
def test_hmax_and_default_edges(shape, capsys):
    """rdr_pair_distance_max within 2 ulp of NumPy's (0 expected: printed), NaN for a date with fewer than two valid points; the
    default bins linspace(0, 0.67 hmax[d], nbins + 1) (:638) give NumPy's counts on edges made from NumPy's own hmax"""
    c = case(**shape)
    want_edges = V.default_edges(c['hmax'], 19)
    assert_off_edges(c['x'], c['y'], want_edges)
    pv = V.pair_variogram(c['x'], c['y'], c['v'])
    assert np.array_equal(np.isnan(pv.hmax), np.isnan(c['hmax']))
    ok = ~np.isnan(c['hmax'])
    ulps = np.abs(pv.hmax[ok] - c['hmax'][ok]) / np.spacing(c['hmax'][ok])
    with capsys.disabled():
        print(f'\n  hmax: largest difference from NumPy {ulps.max() if ulps.size else 0.0:g} ulp', end='')
    assert np.all(ulps <= 2)
    assert pv.edges.shape == want_edges.shape and np.array_equal(np.isnan(pv.edges), np.isnan(want_edges))
    assert np.allclose(pv.edges[ok], want_edges[ok], rtol=4 * 2.0 ** -52, atol=0)
    usable = V._usable_rows(want_edges)                       # a date without pairs has no row of its own and no pair to bin
    assert_sums(pv.count, pv.lag_sum, pv.gamma_sum, numpy_variogram(c['x'], c['y'], c['v64'], usable))
    assert np.all(pv.count[~ok] == 0)


def test_many_workgroups_twice(monkeypatch):
    """N = 1500: 6 tiles, 21 tile pairs = 21 workgroups whose partials a second kernel adds.  Two calls give identical bytes for count;
    the f64 sums of both are within the bound (bit-equality is not required: LDS atomics arrive in any order).  Then the same with the
    grid capped at 4 workgroups, each of which walks 5 or 6 tile pairs."""
    c = case(1500, d=2, holes=False)
    a = call_host(c); b = call_host(c)
    assert a.count.tobytes() == b.count.tobytes()
    for pv in (a, b):
        assert_sums(pv.count, pv.lag_sum, pv.gamma_sum, c['want'])
    monkeypatch.setenv('RAIDER_HIP_VARIOGRAM_GRID', '4')
    few = call_host(c)
    assert few.count.tobytes() == a.count.tobytes()
    assert_sums(few.count, few.lag_sum, few.gamma_sum, c['want'])
    want_h = c['hmax']
    got_h = V.pair_variogram(c['x'], c['y'], c['v'], nbins=3).hmax
    assert np.all(np.abs(got_h - want_h) <= 2 * np.spacing(want_h))


# ---- the C ABI's refusals --------------------------------------------------------------------------------------------------------
def _abi(loc):
    import torch
    ctx = R.Context.default()
    n, nd, nb = 5, 3, 4
    host = dict(x=np.arange(n, dtype=np.float64), y=np.zeros(n), v=np.ones((nd, n)), edges=np.linspace(0.5, 4.5, nb + 1),
                bad_edges=np.linspace(4.5, 0.5, nb + 1), rows2=np.tile(np.linspace(0.5, 4.5, nb + 1), (2, 1)),
                count=np.full((nd, nb), -7, dtype=np.int64), lag=np.full((nd, nb), -7.0), gam=np.full((nd, nb), -7.0), hmax=np.full(nd, -7.0))
    if loc == L.RDR_DEVICE:
        bufs = {k: torch.from_numpy(a).cuda() for k, a in host.items()}
        torch.cuda.synchronize()
        read = lambda k: bufs[k].cpu().numpy()
    else:
        bufs = {k: a.copy() for k, a in host.items()}
        read = lambda k: bufs[k]
    return ctx, n, nd, nb, host, bufs, read


@pytest.mark.parametrize('loc', [L.RDR_HOST, L.RDR_DEVICE], ids=['host', 'device'])
def test_error_texts_and_untouched_outputs(loc):
    ctx, n, nd, nb, host, bufs, read = _abi(loc)
    p = lambda k: L.ptr(bufs[k])
    vg = lambda n_=n, nd_=nd, e='edges', rows=1, nb_=nb, loc_=loc: ctx.lib.rdr_pair_variogram(
        ctx.handle, p('x'), p('y'), n_, p('v'), nd_, p(e), rows, nb_, p('count'), p('lag'), p('gam'), loc_)
    hm = lambda n_=n, nd_=nd, loc_=loc: ctx.lib.rdr_pair_distance_max(ctx.handle, p('x'), p('y'), n_, p('v'), nd_, p('hmax'), loc_)
    for call, text in ((lambda: vg(n_=1), 'n must be 2 .. 2^20 points (got 1)'), (lambda: hm(n_=1), 'n must be 2 .. 2^20 points (got 1)'),
                       (lambda: vg(n_=(1 << 20) + 1), 'n must be 2'), (lambda: vg(nd_=0), 'nd must be 1 .. 4096 dates (got 0)'),
                       (lambda: hm(nd_=4097), 'nd must be 1 .. 4096 dates (got 4097)'),
                       (lambda: vg(nb_=65), 'nbins must be 1 .. 64 (got 65)'), (lambda: vg(nb_=0), 'nbins must be 1 .. 64 (got 0)'),
                       (lambda: vg(e='bad_edges'), 'edge row 0 is not strictly ascending at index 1'),
                       (lambda: vg(e='rows2', rows=2), 'nedge_rows must be 1 or nd = 3 (got 2)'),
                       (lambda: vg(loc_=2), 'loc must be RDR_HOST or RDR_DEVICE'), (lambda: hm(loc_=-1), 'loc must be RDR_HOST or RDR_DEVICE')):
        assert call() == L.RDR_ERR_INVALID
        assert text in L.last_error(ctx.handle), (text, L.last_error(ctx.handle))
    assert ctx.lib.rdr_pair_variogram(ctx.handle, p('x'), None, n, p('v'), nd, p('edges'), 1, nb, p('count'), p('lag'), p('gam'), loc) == L.RDR_ERR_INVALID
    assert 'NULL argument' in L.last_error(ctx.handle)
    ctx.synchronize()
    for k in ('count', 'lag', 'gam', 'hmax'):                       # the sentinels are still there
        assert np.array_equal(read(k), host[k]), k
    assert vg() == L.RDR_OK and hm() == L.RDR_OK                    # and the same buffers make a valid call
    ctx.synchronize()
    want = numpy_variogram(host['x'], host['y'], host['v'], host['edges'][None, :])
    assert_sums(read('count'), read('lag'), read('gam'), want)
    assert np.array_equal(read('hmax'), np.full(nd, 4.0))
    with pytest.raises(ValueError, match='not strictly ascending'):       # the Python layer hands tensor edges to the library's check
        import torch
        dev = lambda a: torch.from_numpy(np.array(a)).cuda()
        V.pair_variogram(dev(host['x']), dev(host['y']), dev(host['v']), edges=dev(host['bad_edges']))


# ---- the chain, and the reference's own results ------------------------------------------------------------------------------------
def test_station_chain_matches_its_numpy_restatement():
    """station_variograms = utm_common_center + deramp + pair_variogram (default bins) + fit per date: the binned variogram equals the
    NumPy restatement on the same metres and the same deramped values; a date below the density threshold is empty"""
    rng = np.random.default_rng(5)
    lon = rng.uniform(-118.4, -116.9, 48); lat = rng.uniform(33.2, 34.4, 48)
    v = 2.3 + 0.02 * rng.standard_normal((3, 48)) + 0.05 * (lon + 117.5)
    v[0, 3] = np.nan; v[2, 9:] = np.nan                                  # date 2: nine stations
    sv = V.station_variograms(lon, lat, v)
    x, y = V.utm_common_center(lon, lat)
    assert np.array_equal(sv.x, x) and 3.6e6 < y.min() < y.max() < 3.9e6 and 3.5e5 < x.min() < x.max() < 6.5e5      # zone 11
    vv = v.copy(); vv[2] = np.nan
    dr = V.deramp(x, y, vv)
    edges = V._usable_rows(V.default_edges(numpy_hmax(x, y, dr), 19))
    assert_off_edges(x, y, edges)
    count, lag, gam = numpy_variogram(x, y, dr, edges)
    assert_sums(sv.variogram.count, sv.variogram.lag_sum, sv.variogram.gamma_sum, (count, lag, gam))
    for d in range(2):
        h, g = sv.binned[d]
        assert h.size == (count[d] > 0).sum() and sv.fits[d] is not None and sv.fits[d].params.shape == (3,)
    assert sv.binned[2][0].size == 0 and sv.fits[2] is None


@pytest.mark.parametrize('s', ['a', 'b', 'c'])
def test_against_the_reference(s):
    """tests/golden/g20_variogram.npz (tools/gen_golden_variogram.py): VariogramAnalysis._get_samples .. _fit_vario of the reference on 40
    points = 780 pairs, below the 1000 at which it starts to sample - it used every pair.
      * bin counts: exact;
      * hExp / expVario: relative (m + 4) * 2^-52 (the sums' bound) + 1e-15 (what nanmean's own summation order may differ by);
      * fitted (range, sill, nugget): within 10 x the spread of the REFERENCE's fit under a relative 1e-12 perturbation of its binned
        input, measured by the generator over 32 perturbed runs and stored as <s>_fit_spread.  Measured spreads, relative to the
        parameters: a (2.1e-8, 1.7e-9, 9.9e-13), b (6.6e-9, 7.8e-10, 1.0e-12), c (9.7e-13, 1.4e-12, 1.0e-12); the tolerance is ten times
        that, per set and parameter."""
    g = np.load(GOLDEN)
    x, y, v = g['x'], g['y'], g[f'{s}_values']
    assert_off_edges(x, y, g[f'{s}_edges'][None, :])
    pv = V.pair_variogram(x, y, v)
    assert abs(pv.hmax[0] - g[f'{s}_hmax']) <= 2 * np.spacing(g[f'{s}_hmax'])
    count = g[f'{s}_count']
    assert np.array_equal(pv.count[0], count) and count.sum() > 600
    h, gam = pv.binned(0)
    m = count[count > 0]
    tol = (m + 4) * 2.0 ** -52 + 1e-15
    assert np.all(np.abs(h - g[f'{s}_hexp']) <= tol * g[f'{s}_hexp'])
    assert np.all(np.abs(gam - g[f'{s}_vexp']) <= tol * g[f'{s}_vexp'])
    fit = V.fit_variogram(h, gam)
    assert np.all(np.abs(fit.params - g[f'{s}_fit']) <= 10 * g[f'{s}_fit_spread']), (fit.params, g[f'{s}_fit'], g[f'{s}_fit_spread'])


def test_below_the_density_threshold_is_empty():
    """nine stations: the reference's _get_samples passes the empty sample (golden: few_samples = 0 at few_n = 9, threshold 10)"""
    g = np.load(GOLDEN)
    assert int(g['few_n']) == 9 and int(g['few_samples']) == 0 and int(g['density_threshold']) == 10
    lon = np.linspace(-117.9, -117.1, 9); lat = np.linspace(33.3, 34.1, 9) + 0.01 * np.arange(9) ** 2
    sv = V.station_variograms(lon, lat, g['a_values'][:9])
    assert sv.variogram.count.sum() == 0 and sv.binned[0][0].size == 0 and sv.fits[0] is None
    sv = V.station_variograms(lon, lat, g['a_values'][:9], density_threshold=9, fit=False)
    assert sv.variogram.count.sum() > 0
