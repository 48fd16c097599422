"""GPU: the three kernels every delay starts from (csrc/producer_kernels.h: producer_kernel, ecmwf_levels_kernel, pressure_levels_kernel)
against the references of tests/front_end_exact.py, on the paths the goldens and the oracle scenes never reach: a second trip of each
grid-stride loop, every strip arrangement of the NaN fill and of the suffix scan with and without the pad level, queries exactly on
model levels, the svp branch temperatures, the tile edges of the transpose.

The launch arithmetic of the three host entries (raider_hip.hip) is restated in `_Launch`, its multipliers READ OUT of the source, and
every size is derived from the CU count; EVERY CASE FIRST ASSERTS FROM IT THAT IT REACHES THE PATH IT IS NAMED FOR: after a retuned
launch a case fails and says so, it does not pass on another path.

What is asserted.  Producer: t, p and hydro bit for bit, e and wet bit for bit except where an svp behind them lies within 4 float64
ulps of a float32 rounding tie (front_end_exact: none in these scenes so far; the count is printed), and BOTH totals against the
long-double suffix sums of the device's own point-wise cube: |total - S| <= c eps A, A = 1e-6 sum |term|, with

    c = 2 (a term: the height difference and the product; the halving is exact) + 6 (shuffle steps of the scan in a strip)
      + ceil(nzo / 64) (the carry: one addition per strip on the way down) + 1 (the scale 1e-6)

roundings on the longest path (17 at 512 levels), eps = 2^-52: twice the first-order bound c u A, which leaves room for the second
order and for the reference's own 0.13 eps A.  The top level's totals are exactly 0.  Hybrid levels: |zs - exact| <= 4 k64 eps C per
level (k64: what NumPy's float64 evaluation of the same formulas loses, measured on the host by front_end_exact.measure_k64 - never on
the device; 4: the device's log / exp / cos may differ from glibc's by an ulp) and p within 1 ulp.  Pressure levels: moved values
bit for bit, heights of kinds 0 and 1 within H_ATOL of the 40-digit geo_to_ht."""
import itertools
import math
import re
from pathlib import Path

import numpy as np
import pytest

from tests import front_end_exact as X                    # (imports mpmath: its absence is an error here, not a skip)

pytestmark = pytest.mark.gpu

EPS = X.EPS
H_ATOL = 1e-9                                            # tests/test_gpu_pressure_levels.py
G0 = 9.80665


# ---- the launch arithmetic --------------------------------------------------------------------------------------------------------
class _Launch:
    def __init__(self, cus):
        src = (Path(__file__).resolve().parent.parent / 'raider_amd' / 'csrc' / 'raider_hip.hip').read_text()
        pats = dict(producer=r'std::min<int64_t>\(\(ncol \+ 3\) / 4, \(int64_t\)c->num_cus \* (\d+)\)',
                    ecmwf=r'ecmwf_levels_kernel, dim3\(grid_for\(ncol, 256, c->num_cus \* (\d+)\)\), dim3\(256\)',
                    pressure=r'pressure_levels_kernel, dim3\(\(unsigned\)std::max<int64_t>\(1, std::min<int64_t>\(ntiles, \(int64_t\)c->num_cus \* (\d+)\)\)\), dim3\(256\)')
        self.cus = cus
        self.per_cu = {}
        for k, pat in pats.items():
            m = re.search(pat, src)
            assert m, f'the launch of the {k} kernel is no longer written as this module restates it: restate the schedule model'
            self.per_cu[k] = int(m.group(1))

    def producer_grid(self, ncol):                       # four waves per workgroup, one column per wave and trip
        return max(1, min((ncol + 3) // 4, self.cus * self.per_cu['producer']))

    def producer_trips(self, ncol):
        return -(-ncol // (4 * self.producer_grid(ncol)))

    def ecmwf_trips(self, ncol):                         # one column per thread, 256 threads per workgroup
        g = max(1, min(-(-ncol // 256), self.cus * self.per_cu['ecmwf']))
        return -(-ncol // (256 * g))

    @staticmethod
    def tiles(nlev, ny, nx):
        return ny * (-(-nx // 32)) * (-(-nlev // 32))

    def pressure_trips(self, nlev, ny, nx):
        n = self.tiles(nlev, ny, nx)
        return -(-n // max(1, min(n, self.cus * self.per_cu['pressure'])))


@pytest.fixture(scope='module')
def cus():
    from raider_amd._lib import Context
    return Context.default().device_info()[1]


@pytest.fixture(scope='module')
def launch(cus):
    return _Launch(cus)


@pytest.fixture(scope='module')
def k64():
    return X.measure_k64()['k64']


# ---- producer: helpers ------------------------------------------------------------------------------------------------------------
def _grid_of(n):
    """(ny, nx) with ny nx = n and the fewest rows >= 2 (a cube axis needs two nodes), None for a prime"""
    for ny in range(2, math.isqrt(n) + 1):
        if n % ny == 0:
            return ny, n // ny
    return None


def _produce(zs, p, t, hum, kind, new_z, zmin=-100.0, as_given=False):
    """(ncol, nlev) columns -> dict of (ncol, nzo) arrays and the output heights.  The kernel sees a flat list of columns; the grid they
    are handed over in is ny x nx with the fewest rows that divide their number (a cube axis needs two nodes, so never 1 x ncol) - a
    prime number of columns is made up with copies of the last one, dropped again here, unless as_given asks for exactly these."""
    from raider_amd.weather import cubes_from_model_levels
    ncol = n = zs.shape[0]
    while _grid_of(n) is None:
        n += 1
    assert n == ncol or not as_given, f'{ncol} columns make no grid'
    ny, nx = _grid_of(n)
    take = np.minimum(np.arange(n), ncol - 1)
    m = cubes_from_model_levels(0.01 * np.arange(nx), 33.0 + 0.01 * np.arange(ny), *(np.ascontiguousarray(v[take].reshape(ny, nx, -1)) for v in (zs, p, t, hum)), kind,
                                new_z, zmin=zmin, return_state=True)
    wet, hyd = m.pointwise.read()
    wt, ht = m.total.read()
    assert wet.dtype == np.float32 and wt.dtype == np.float64 and wet.shape[:2] == (ny, nx)
    flat = lambda v: np.ascontiguousarray(np.asarray(v).reshape(n, -1)[:ncol])
    return dict(zs=np.asarray(m.zs), t=flat(m.t), p=flat(m.p), e=flat(m.e), wet=flat(wet), hydro=flat(hyd), wet_total=flat(wt), hydro_total=flat(ht))


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _check_state(got, ref, sel=slice(None), what=''):
    """t, p, hydro bit for bit; e and wet bit for bit outside the flagged ties.  Returns the number of flagged values."""
    assert np.array_equal(got['zs'], ref['zs']), what
    for k in ('t', 'p', 'hydro'):
        assert _bits_equal(got[k][sel], ref[k]), f'{what}: {k} differs in {int((got[k][sel] != ref[k]).sum())} values'
    keep = ~ref['flagged']
    for k in ('e', 'wet'):
        bad = (got[k][sel].view(np.uint32) != ref[k].view(np.uint32)) & keep
        assert not bad.any(), f'{what}: {k} differs in {int(bad.sum())} values away from any rounding tie, first at {tuple(np.argwhere(bad)[0])}'
    return int(ref['flagged'].sum())


def _check_totals(got, what=''):
    """both totals against the exact suffix sums of the device's own point-wise cube; returns the worst |total - S| / (eps A)"""
    nzo = got['wet'].shape[-1]
    c = 2 + 6 + (nzo + 63) // 64 + 1                      # derived in the module docstring: not a tuned figure
    worst = 0.0
    for name in ('wet', 'hydro'):
        f, tot = got[name], got[f'{name}_total']
        assert np.isfinite(f).all() and np.isfinite(tot).all(), f'{what}: {name} is not finite'
        assert np.all(tot[..., -1] == 0.0), f'{what}: the top level of {name}_total is not exactly 0'
        S, A = X.ztd_exact(f, got['zs'])
        r = X.ztd_ratio(tot, S, A)
        worst = max(worst, float(r.max()))
        assert r.max() <= c, f'{what}: |{name}_total - exact| reaches {r.max():.3g} eps A (bound {c})'
    return worst


def _atmosphere(z, kind, rng=None):
    """t, p, humidity at heights z; t carries a ripple so that neighbouring levels never lie on one line"""
    t = np.maximum(288.0 - 0.0065 * z, 210.0) + 0.7 * np.sin(z / 173.0)
    p = 101000.0 * np.exp(-z / 7700.0)
    hum = 0.010 * np.exp(-z / 2500.0) if kind == 'q' else 70.0 * np.exp(-z / 8000.0) + 1.0
    if rng is not None:
        t = t + rng.normal(0, 0.3, z.shape)
        hum = hum * rng.uniform(0.7, 1.3, z.shape)
    return t, p, hum


# ---- producer: the second trip of the column loop -------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['q', 'rh'])
def test_producer_second_trip_of_the_column_loop(launch, kind):
    """32 CUs + 7 columns: seven waves take a second column into the LDS buffers their first one used (o_z is written once, before
    the loop).  Every fifth column carries a hole whose kind cycles (a NaN level, a dead column, a NaN top): period 15, coprime to the
    stride, so among the seven waves one meets a hole and then none, another the reverse.  Bit for bit the same columns submitted in
    two batches of one trip each; equal to producer_exact on a stride sample of more than 512 columns with the first and last 16."""
    one_trip = 4 * launch.cus * launch.per_cu['producer']
    ncol, nlev = one_trip + 7, 6
    assert launch.producer_trips(ncol) == 2 and launch.producer_trips(one_trip) == 1 and launch.producer_grid(ncol) * 4 == one_trip
    assert math.gcd(15, one_trip) == 1, 'the hole pattern must be coprime to the column stride: choose another period'
    rng = np.random.default_rng(11 if kind == 'q' else 12)
    zs = rng.uniform(-80.0, 200.0, (ncol, 1)) + np.array([0.0, 300.0, 1500.0, 5000.0, 12000.0, 30000.0]) * rng.uniform(0.9, 1.1, (ncol, nlev))
    assert np.all(np.diff(zs, axis=1) > 0)
    t, p, hum = _atmosphere(zs, kind, rng)
    cols = np.arange(ncol)
    hole = np.where(cols % 5 == 0, (cols // 5) % 3, -1)
    t[hole == 0, 2] = np.nan                               # a NaN level: an interior run
    t[hole == 1, :] = np.nan                               # a dead column
    p[hole == 2, 4:] = np.nan                              # a NaN top
    pairs = [(hole[c], hole[c + one_trip]) for c in range(7)]            # what the seven waves see in their two trips
    assert any(a >= 0 and b < 0 for a, b in pairs) and any(a < 0 and b >= 0 for a, b in pairs)   # a hole, then none - and the reverse
    new_z = np.array([-50.0, 400.0, 2500.0, 9000.0, 20000.0]) if kind == 'q' else np.array([-100.0, 400.0, 2500.0, 9000.0, 20000.0])
    whole = _produce(zs, p, t, hum, kind, new_z, as_given=True)
    assert whole['t'].shape == (ncol, 6 if kind == 'q' else 5)
    cut = next(k for k in range(one_trip, one_trip - 64, -1) if _grid_of(k) and _grid_of(ncol - k))      # two batches that make grids, one trip each
    assert launch.producer_trips(cut) == 1 and launch.producer_trips(ncol - cut) == 1
    a = _produce(zs[:cut], p[:cut], t[:cut], hum[:cut], kind, new_z, as_given=True)
    b = _produce(zs[cut:], p[cut:], t[cut:], hum[cut:], kind, new_z, as_given=True)
    for k in ('t', 'p', 'e', 'wet', 'hydro', 'wet_total', 'hydro_total'):
        assert _bits_equal(whole[k], np.concatenate([a[k], b[k]])), f'{k}: one launch of two trips differs from two launches of one'
    sel = np.unique(np.concatenate([np.arange(16), np.arange(ncol - 16, ncol), np.linspace(0, ncol - 1, 512).astype(np.int64)]))
    assert sel.size >= 512 and {0, 1, 2} <= set(hole[sel])
    ref = X.producer_exact(zs[sel], p[sel], t[sel], hum[sel], kind, new_z)
    nflag = _check_state(whole, ref, sel, f'second trip ({kind})')
    worst = _check_totals(whole, f'second trip ({kind})')
    print(f'producer second trip ({kind}): {ncol} columns, {sel.size} checked against producer_exact, {nflag} flagged; totals within {worst:.3g} eps A')


# ---- producer: the strips of the fill and of the scan ---------------------------------------------------------------------------
def _levels_for(segs, nlev):
    """Model levels, as fractional positions on the output-level index, that leave exactly the output levels of `segs` (inclusive
    index ranges) valid: a level half a step outside either end of every segment, one NaN level inside every gap, the rest spread
    inside the segments off the integers.  Returns (positions ascending, which of them carry NaN)."""
    pos, hole = [], []
    fixed = 2 * len(segs) + len(segs) - 1
    spare = nlev - fixed
    assert spare >= 0
    width = [e - s + 1 for s, e in segs]
    share = [spare * w // sum(width) for w in width]
    share[int(np.argmax(width))] += spare - sum(share)
    for i, (s, e) in enumerate(segs):
        if i:
            pos.append(0.5 * (segs[i - 1][1] + s) + 0.125); hole.append(True)
        pos.append(s - 0.5); hole.append(False)
        for k in range(share[i]):
            pos.append(s - 0.5 + (e - s + 1) * (k + 0.61) / (share[i] + 1)); hole.append(False)
        pos.append(e + 0.5); hole.append(False)
    assert len(pos) == nlev and all(b > a for a, b in zip(pos, pos[1:]))
    return np.array(pos), np.array(hole)


def _strip_columns(nz):
    """{name: (valid output-index segments, t wholly NaN)} for one output level count"""
    full = [(0, nz - 1)]
    cols = dict(plain=(full, False), dead_t=(full, True))
    if nz >= 128:
        cols['lead_70'] = ([(70, nz - 1)], False)                                            # a leading run longer than a strip
        cols['across'] = ([(0, 59), (68, 123), (132, nz - 1)] if nz >= 200 else [(0, 59), (68, nz - 1)], False)   # runs across 63|64 (and 127|128)
        cols['run_71'] = ([(0, 19), (91, nz - 1)], False)                                     # an interior run longer than a strip
    else:
        cols['lead'] = ([(nz - 5, nz - 1)], False)
        cols['interior'] = ([(0, 9), (41, nz - 1)], False)
        cols['trail'] = ([(0, nz // 2)], False)
    if nz == 65:
        cols['only_64'] = ([(64, 64)], False)                                                 # first = last = the one level of strip 1
        cols['run_to_64'] = ([(0, 49), (64, 64)], False)                                      # the upward search leaves strip 0
    if nz >= 200:
        cols['only_strip_2'] = ([(140, 150)], False)                                          # first / last: no valid level in strips 0 and 1
        cols['trail_strip_2'] = ([(0, 149)], False)
    elif nz >= 128:
        cols['only_strip_1'] = ([(100, 110)], False)
        cols['trail_strip_1'] = ([(0, 99)], False)
    return cols


def _runs(mask):
    """[(first, last)] of the True runs of a 1-D mask"""
    d = np.diff(np.concatenate([[0], mask.astype(np.int8), [0]]))
    return list(zip(np.nonzero(d == 1)[0].tolist(), (np.nonzero(d == -1)[0] - 1).tolist()))


@pytest.mark.parametrize('nlev', [12, 70])
@pytest.mark.parametrize('pad', [0, 1])
@pytest.mark.parametrize('nz', [64, 65, 128, 200, 511])
def test_producer_fill_and_scan_strips(nz, pad, nlev):
    """fillna_col walks the nz resampled levels in strips of 64 (on o_p + pad), the suffix scan the nzo = nz + pad output levels: runs
    that start, end and span strip boundaries, valid levels only in a later strip, with and without the pad level.  Twice in one
    context: the second run sees the LDS the first one left behind."""
    kind = 'q' if nlev == 12 else 'rh'
    z0, dz = (-50.0, 100.0) if pad else (-100.0, 100.0)
    new_z = z0 + dz * np.arange(nz)
    spec = _strip_columns(nz)
    names = list(spec)
    zs = np.empty((len(names), nlev)); t = np.empty_like(zs); p = np.empty_like(zs); hum = np.empty_like(zs)
    for c, name in enumerate(names):
        segs, dead = spec[name]
        pos, hole = _levels_for(segs, nlev)
        zs[c] = z0 + dz * pos
        t[c], p[c], hum[c] = _atmosphere(zs[c] + 37.0 * c, kind)
        t[c, hole] = np.nan; p[c, hole] = np.nan
        if dead:
            t[c, :] = np.nan
    ref = X.producer_exact(zs, p, t, hum, kind, new_z, zmin=-100.0)
    # the paths, from the reference's unfilled state
    nzo = nz + pad
    assert ref['t'].shape == (len(names), nzo) and (nz + 63) // 64 == {64: 1, 65: 2, 128: 2, 200: 4, 511: 8}[nz]
    for c, name in enumerate(names):
        segs, dead = spec[name]
        want = np.ones(nz, bool)
        for s, e in segs:
            want[s:e + 1] = False
        assert np.array_equal(np.isnan(ref['p_u'][c]), want), f'{name}: the resampled column does not have the runs it is named for'
        assert np.array_equal(np.isnan(ref['t_u'][c]), want | dead) and np.array_equal(np.isnan(ref['e_u'][c]), want | dead)
    runs = {name: _runs(np.isnan(ref['p_u'][c])) for c, name in enumerate(names)}
    assert np.isfinite(ref['p_u'][names.index('dead_t')]).all() and ref['t'][names.index('dead_t')].min() == np.float32(1e16)
    if nz >= 128:
        assert runs['lead_70'] == [(0, 69)] and (60, 67) in runs['across'] and runs['run_71'] == [(20, 90)]
    if nz >= 200:
        assert (124, 131) in runs['across'] and runs['only_strip_2'] == [(0, 139), (151, nz - 1)] and runs['trail_strip_2'] == [(150, nz - 1)]
    if nz == 65:
        assert runs['only_64'] == [(0, 63)] and runs['run_to_64'] == [(50, 63)]
    for rep in range(2):
        got = _produce(zs, p, t, hum, kind, new_z, zmin=-100.0)
        assert got['t'].shape[1] == nzo
        nflag = _check_state(got, ref, what=f'nz {nz} pad {pad} nlev {nlev} run {rep}')
        worst = _check_totals(got, f'nz {nz} pad {pad} nlev {nlev} run {rep}')
    print(f'producer strips nz {nz} pad {pad} nlev {nlev}: {len(names)} columns, {nflag} flagged; totals within {worst:.3g} eps A (bound {2 + 6 + (nzo + 63) // 64 + 1})')


# ---- producer: queries exactly on model levels, the branch temperatures of svp --------------------------------------------------------
@pytest.mark.parametrize('kind', ['q', 'rh'])
@pytest.mark.parametrize('pad', [0, 1])
def test_producer_ties(pad, kind):
    """interpolate_1d takes the interval ABOVE a query that equals a model level (x < xs[mid] is false on equality): on the lowest level
    the query is valid and returns y0 exactly, on an interior one y0 of the upper interval exactly, on the top one it is out of range:
    NaN, then the fill.  The temperatures there are 250.15 K and 273.15 K - where find_svp changes branch - and one ulp on either side."""
    z_low = -20.0 if pad else -100.0
    z_mid, z_top = 4000.0, 26000.0
    new_z = np.array([z_low, 700.0, z_mid, 9000.0, z_top, 31000.0])
    T = [np.nextafter(250.15, 0.0), 250.15, np.nextafter(250.15, 1e3), np.nextafter(273.15, 0.0), 273.15, np.nextafter(273.15, 1e3)]
    ncol, nlev = 12, 7
    rng = np.random.default_rng(40 + pad)
    zs = np.empty((ncol, nlev))
    for c in range(ncol):
        zs[c] = [z_low, 350.0 + 20.0 * c, 2100.0 + 31.0 * c, z_mid, 8000.0 + 57.0 * c, 15000.0 + 11.0 * c, z_top]
    t, p, hum = _atmosphere(zs, kind, rng)
    for c in range(ncol):
        t[c, 0], t[c, 3], t[c, 6] = T[c % 6], T[(c + 2) % 6], T[(c + 4) % 6]
    ref = X.producer_exact(zs, p, t, hum, kind, new_z, zmin=-100.0)
    j = pad                                                 # output index of new_z[0]
    assert np.array_equal(ref['t_u'][:, 0], t[:, 0].astype(np.float32)) and np.array_equal(ref['t_u'][:, 2], t[:, 3].astype(np.float32))   # valid, y0 exactly
    assert np.array_equal(ref['p_u'][:, 2], p[:, 3].astype(np.float32))
    assert np.isnan(ref['t_u'][:, 4:]).all() and np.isfinite(ref['t_u'][:, :4]).all()                                            # on the top level: out of range
    assert np.all(ref['t'][:, j + 4:] == np.float32(1e16)) and np.all(ref['p'][:, j + 4:] == 0) and ref['t'].shape[1] == 6 + pad
    assert ref['svp_tie'].min() >= X.TIE_ULPS               # the branch temperatures themselves are far from any tie
    got = _produce(zs, p, t, hum, kind, new_z, zmin=-100.0)
    nflag = _check_state(got, ref, what=f'ties pad {pad} {kind}')
    worst = _check_totals(got, f'ties pad {pad} {kind}')
    print(f'producer ties pad {pad} {kind}: {nflag} flagged; totals within {worst:.3g} eps A')


# ---- hybrid model levels ----------------------------------------------------------------------------------------------------------
def _single_level_state():
    """one model level (the lev == 1 branch alone: dlogP = log(P1 / 0.1), alpha = log 2): its height is TRd log 2 / g0 above the
    surface, C about 5.5 km - the case where a less-than-double alpha shows"""
    rng = np.random.default_rng(21)
    ny, nx = 5, 3
    return dict(z=np.zeros((ny, nx), np.float32), lnsp=np.log(rng.uniform(50000.0, 108000.0, (ny, nx))).astype(np.float32),
                t=rng.uniform(230.0, 300.0, (1, ny, nx)).astype(np.float32), q=rng.uniform(0.0, 0.01, (1, ny, nx)).astype(np.float32),
                lats=np.array([-90.0, -41.5, 0.0, 63.25, 90.0], np.float32), a=np.array([0.0, 0.0]), b=np.array([0.0, 1.0]))


def _hybrid_gpu(s):
    from raider_amd.weather import ecmwf_model_levels
    return ecmwf_model_levels(s['z'], s['lnsp'], s['t'], s['q'], s['lats'], s['a'], s['b'])


@pytest.mark.parametrize('name', ['block', 'synthetic', 'single_level'])
def test_hybrid_levels_against_exact(k64, name):
    """per level |zs - exact| <= 4 k64 eps C, p within 1 ulp; a column without a surface pressure is NaN, and only that column"""
    if name == 'single_level':
        s = _single_level_state()
        p_x, zs_x, C = X.ecmwf_levels_exact(s['z'], s['lnsp'], s['t'], s['q'], s['lats'], s['a'], s['b'])
    else:
        s, (p_x, zs_x, C) = X.hybrid_cases()[name]
    p, zs = _hybrid_gpu(s)
    ok = np.isfinite(zs_x)
    if name == 'synthetic':
        lat = s['lats'].tolist()
        assert 90.0 in lat and -90.0 in lat and 0.0 in lat and s['z'].min() < 0 and (~ok).sum() == s['t'].shape[0]
        sp = np.exp(s['lnsp'][np.isfinite(s['lnsp'])].astype(np.float64))
        assert sp.min() < 50100.0 and sp.max() > 107900.0
    else:
        assert ok.all()
    assert np.array_equal(np.isnan(zs), ~ok) and np.array_equal(np.isnan(p), ~ok)
    assert np.all(np.abs(p - p_x)[ok] <= np.spacing(np.abs(p_x[ok]))), 'p is more than 1 ulp from the exact half-level pressure'
    ratio = np.abs(zs - zs_x)[ok] / (EPS * C[ok])
    print(f'hybrid levels {name} {s["t"].shape}: worst |zs - exact| = {ratio.max():.4g} eps C ({np.abs(zs - zs_x)[ok].max():.3g} m); bound 4 k64 = {4 * k64:.4g}')
    assert ratio.max() <= 4 * k64


def _odd_grid(ncol):
    """ny x nx = ncol with nx odd, > 1 and below ny"""
    best = None
    for nx in range(3, math.isqrt(ncol) + 1, 2):
        if ncol % nx == 0 and ncol // nx != nx:
            best = nx
    assert best, f'{ncol} columns have no odd factor to make a grid of: choose another tail than 37'
    return ncol // best, best


def test_hybrid_levels_second_trip_of_the_column_loop(launch, k64):
    """2048 CUs + 37 columns on an ny x nx grid with nx odd and far from ny (lats[i / nx] differs from lats[i / ny] for nearly every
    column): 37 threads take a second column.  Bit for bit the same columns run in two row blocks of one trip each; within the bound of
    the NumPy float64 evaluation on a stride sample that holds all 37."""
    from oracle import raider_oracle as O
    one_trip = 256 * launch.cus * launch.per_cu['ecmwf']
    ncol = one_trip + 37
    ny, nx = _odd_grid(ncol)
    assert nx % 2 == 1 and nx != ny and launch.ecmwf_trips(ncol) == 2
    nlev = 3
    a, b = np.array([0.0, 5000.0, 3000.0, 0.0]), np.array([0.0, 0.1, 0.6, 1.0])
    rng = np.random.default_rng(5)
    s = dict(z=(G0 * rng.uniform(-400.0, 5000.0, (ny, nx))).astype(np.float32), lnsp=np.log(rng.uniform(50000.0, 105000.0, (ny, nx))).astype(np.float32),
             t=rng.uniform(210.0, 300.0, (nlev, ny, nx)).astype(np.float32), q=rng.uniform(0.0, 0.02, (nlev, ny, nx)).astype(np.float32),
             lats=np.linspace(-89.0, 89.0, ny).astype(np.float32), a=a, b=b)
    p, zs = _hybrid_gpu(s)
    assert p.shape == (ny, nx, nlev) and np.isfinite(zs).all()
    h = ny // 2
    for r0, r1 in ((0, h), (h, ny)):
        assert launch.ecmwf_trips((r1 - r0) * nx) == 1
        c = np.ascontiguousarray
        part = dict(z=c(s['z'][r0:r1]), lnsp=c(s['lnsp'][r0:r1]), t=c(s['t'][:, r0:r1]), q=c(s['q'][:, r0:r1]), lats=c(s['lats'][r0:r1]), a=a, b=b)
        pp, zp = _hybrid_gpu(part)
        assert _bits_equal(pp, p[r0:r1]) and _bits_equal(zp, zs[r0:r1]), f'rows {r0}..{r1}: one launch of two trips differs from a launch of one'
    flat = np.unique(np.concatenate([np.linspace(0, ncol - 1, 27).astype(np.int64), np.arange(ncol - 37, ncol)]))
    iy, ix = flat // nx, flat % nx
    mini = (s['z'][iy, ix][:, None], s['lnsp'][iy, ix][:, None], s['t'][:, iy, ix][:, :, None], s['q'][:, iy, ix][:, :, None], s['lats'][iy], a, b)
    p_x, _, C = X.ecmwf_levels_exact(*mini)
    _, h64 = O.ecmwf_model_levels(*mini, dtype=np.float64)
    ratio = np.abs(zs[iy, ix] - h64[:, 0]) / (EPS * C[:, 0])
    print(f'hybrid levels second trip: {ny} x {nx} columns, worst |zs - float64 oracle| = {ratio.max():.4g} eps C on {flat.size} columns; bound 4 k64 = {4 * k64:.4g}')
    assert ratio.max() <= 4 * k64
    assert np.all(np.abs(p[iy, ix] - p_x[:, 0]) <= np.spacing(np.abs(p_x[:, 0]))), 'p is more than 1 ulp from the exact half-level pressure'


# ---- pressure levels --------------------------------------------------------------------------------------------------------------
def _file_layout(v, top_first, rows_desc, cols_desc):
    """(ny, nx, nlev) surface first, ascending -> (nlev, ny, nx) as a file with these orders holds it"""
    f = v.transpose(2, 0, 1)
    if top_first: f = f[::-1]
    if rows_desc: f = f[:, ::-1]
    if cols_desc: f = f[:, :, ::-1]
    return np.ascontiguousarray(f)


def _level_state(nlev, ny, nx, seed):
    """the state a file holds, in the producer's layout: every value distinct, so a moved element shows"""
    rng = np.random.default_rng(seed)
    n = ny * nx * nlev
    uniq = lambda lo, hi: (lo + (hi - lo) * (rng.permutation(n) + rng.uniform(0.1, 0.9, n)) / n).reshape(ny, nx, nlev)
    lat1 = np.linspace(-71.5, 83.25, ny)
    lat2 = lat1[:, None] + 0.01 * np.arange(nx)[None, :]
    return dict(h=uniq(-300.0, 60000.0), p3=uniq(100.0, 105000.0), t=uniq(190.0, 320.0), q=uniq(0.0, 0.03), p1=np.sort(rng.uniform(100.0, 105000.0, nlev))[::-1].copy(),
                lat1=lat1, lat2=lat2)


def _pressure_case(st, kind, p3, lat2, top_first, rows_desc, cols_desc):
    from raider_amd.weather import pressure_level_state
    lay = lambda v: _file_layout(v, top_first, rows_desc, cols_desc)
    height = lay(st['h'] * G0) if kind == 0 else lay(st['h'])
    p = lay(st['p3']) if p3 else (st['p1'][::-1].copy() if top_first else st['p1'])
    if lat2:
        lats = st['lat2'][::-1] if rows_desc else st['lat2']
        lats = np.ascontiguousarray(lats[:, ::-1] if cols_desc else lats)
    else:
        lats = st['lat1'][::-1].copy() if rows_desc else st['lat1']
    got = pressure_level_state(height, p, lay(st['t']), lay(st['q']), lats, height_kind=kind, top_first=top_first, rows_descending=rows_desc, cols_descending=cols_desc)
    want_p = st['p3'] if p3 else np.broadcast_to(st['p1'], st['t'].shape)
    return got, want_p


@pytest.mark.parametrize('nlev', [31, 32, 33, 65])
def test_pressure_levels_tile_edges(launch, nlev):
    """32 x 32 tiles of (x, level) through LDS: one level short of a tile, a full tile, one past it and two tiles plus one, in both tile
    axes.  Geometric heights (kind 2) in all 32 combinations of level / row / column order, 1-D / 3-D pressure and 1-D / 2-D latitudes:
    every output equals the NumPy transpose / flip exactly.  Kinds 0 and 1 in the 8 order combinations: moved fields exact, heights
    within H_ATOL of the 40-digit geo_to_ht."""
    ny = 2
    worst = 0.0
    for nx in (31, 32, 33):
        assert launch.tiles(nlev, ny, nx) == ny * (1 if nx <= 32 else 2) * {31: 1, 32: 1, 33: 2, 65: 3}[nlev] and launch.pressure_trips(nlev, ny, nx) == 1
        st = _level_state(nlev, ny, nx, 100 * nlev + nx)
        for flags in itertools.product((False, True), repeat=5):
            (zs, p, t, q), want_p = _pressure_case(st, 2, *flags)
            assert zs.shape == (ny, nx, nlev)
            assert _bits_equal(zs, st['h']) and np.array_equal(p, want_p) and _bits_equal(t, st['t']) and _bits_equal(q, st['q']), (nlev, nx, flags)
        exact = {False: X.geo_to_ht_exact(st['lat1'][:, None], st['h']), True: X.geo_to_ht_exact(st['lat2'], st['h'])}
        for kind, order in itertools.product((0, 1), itertools.product((False, True), repeat=3)):
            lat2 = kind == 1                                 # kind 0: level list and one latitude per row; kind 1: a pressure field and one latitude per node
            (zs, p, t, q), want_p = _pressure_case(st, kind, lat2, lat2, *order)
            assert np.array_equal(p, want_p) and _bits_equal(t, st['t']) and _bits_equal(q, st['q']), (nlev, nx, kind, order)
            d = float(np.abs(zs - exact[lat2]).max())
            worst = max(worst, d)
            assert d <= H_ATOL, (nlev, nx, kind, order, d)
    print(f'pressure levels nlev {nlev}: worst |zs - exact geo_to_ht| = {worst:.3e} m')


def test_pressure_levels_second_trip_of_the_tile_loop(launch):
    """nx = 33 and nlev = 33 make four tiles per row, so a tile count is a multiple of 4: ny = 4 CUs + 1 rows give 16 CUs + 4 tiles, four
    of them on a second trip of their workgroup (which reuses the LDS tile behind the loop's closing barrier).  Geometric heights, every
    order reversed: exact."""
    nlev = nx = 33
    per_trip = launch.cus * launch.per_cu['pressure']
    ny = per_trip // 4 + 1
    assert launch.tiles(nlev, ny, nx) == 4 * ny and per_trip < 4 * ny <= per_trip + 4 and launch.pressure_trips(nlev, ny, nx) == 2
    st = _level_state(nlev, ny, nx, 9)
    for flags in ((True, True, True, True, True), (False, False, False, False, False)):
        (zs, p, t, q), want_p = _pressure_case(st, 2, *flags)
        assert _bits_equal(zs, st['h']) and np.array_equal(p, want_p) and _bits_equal(t, st['t']) and _bits_equal(q, st['q']), flags
