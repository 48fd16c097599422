"""GPU: every schedule of the zenith-cube gather (build_cube_kernel, cube_kernels.h, driven by build_cube_impl, raider_hip.hip) against
a long-double trilinear interpolant written here, and bit for bit against Cube.interp (interp_points_kernel).

Which path a tile takes - its footprint staged in LDS in one round or in several rounds of U heights, or direct loads UD heights at
a time with a clamped tail; the CLEAN or the guarded instantiation; a second and third trip of the grid-stride loop over tiles; one or
many heights per blockIdx.y chunk - is decided by host heuristics from the output-grid size and the CU count.  `_Sched` restates that
arithmetic (the constants are read out of cube_kernels.h) and EVERY CASE FIRST ASSERTS FROM IT THAT IT REACHES THE PATH IT IS NAMED
FOR: after a retuned heuristic a case fails and says so, it does not pass on another path.  Grid sizes are derived from the CU count.

Reference: `_Ref`, np.longdouble, scipy's semantics (interval g[i] <= v < g[i+1], last cell closed; out of range or NaN -> NaN; weights
((wy wx) wz), corners in lexicographic (y, x, z) order); per point the value and A = sum |v_i| k_i.  Asserted: identical NaN mask, and
|gpu - ref| <= 16 eps64 A (three t's of at most 2 roundings, 3 roundings per weight product, 8 accumulations: about 14 eps of A; a
float64 NumPy restatement without FMA stays within 4.6 eps A of the long-double one over 3e6 random points).  Where long double has no
64-bit mantissa the same bound is checked in exact rationals on a fixed 2000-point sample.  Large outputs are compared on a fixed
stride sample of >= 2e5 points plus every tile-edge row and column; bit identity with Cube.interp covers every point of every case.

Out of scope: the projection branch of the setup kernels, and BUILD_ZCHUNK_MAX - reaching it takes more than 1024 heights on a grid of
>= 8 CUs tiles, several GB of output."""
import fractions
import itertools
import math
import re
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = 2.0 ** -52
BOUND = 16                                   # x eps64 x A, derived in the module docstring
DTYPES = pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])


# ---- constants of the kernel, the device ------------------------------------------------------------------------------------------
def _kernel_constants():
    src = (Path(__file__).resolve().parent.parent / 'raider_amd' / 'csrc' / 'cube_kernels.h').read_text()
    out = {}
    for name in ('BUILD_STAGE_BYTES', 'BUILD_NCOL_MAX', 'BUILD_ZCHUNK_MAX'):
        m = re.search(r'constexpr\s+int\s+%s\s*=\s*(\d+)\s*(?:(<<|\*)\s*(\d+))?\s*;' % name, src)
        assert m, f'{name} is no longer a plain integer constant of cube_kernels.h: restate the schedule model'
        v = int(m.group(1))
        if m.group(2):
            v = v << int(m.group(3)) if m.group(2) == '<<' else v * int(m.group(3))
        out[name] = v
    return out


@pytest.fixture(scope='module')
def K():
    return _kernel_constants()


@pytest.fixture(scope='module')
def cus():
    from raider_amd._lib import Context
    return Context.default().device_info()[1]


# ---- model cubes ------------------------------------------------------------------------------------------------------------------
def _fields(ny, nx, nz, zs, seed):
    """smooth fields with a 7-periodic pattern and noise on top: neighbouring nodes differ by >= 1e-3 relative (asserted), so a wrong
    corner or weight shows 10 orders above the bound"""
    rng = np.random.default_rng(seed)
    iy, ix, iz = np.ogrid[:ny, :nx, :nz]
    pat = lambda a, b, c: 1.0 + 0.1 * (((a * iy + b * ix + c * iz) % 7) / 7.0 - 0.5)
    wet = (0.25 + 0.02 * np.sin(0.05 * iy + 0.03 * ix)) * np.exp(-zs / 2500.0)[None, None, :] * pat(1, 3, 5) * (1.0 + 1e-3 * rng.uniform(-1, 1, (ny, nx, nz)))
    hyd = (2.3 + 0.1 * np.cos(0.04 * iy - 0.02 * ix)) * np.exp(-zs / 8000.0)[None, None, :] * pat(2, 1, 3) * (1.0 + 1e-3 * rng.uniform(-1, 1, (ny, nx, nz)))
    return wet, hyd


def _model(name):
    """(ys, xs, zs ascending, wet, hydro of shape (ny, nx, nz) in float64)"""
    rng = np.random.default_rng(7)
    if name == 'M1':                         # y non-uniform, x uniform, z non-uniform from below 0 m to 40 km
        ys = 30.0 + np.concatenate([[0.0], np.cumsum(0.10 + 0.08 * rng.random(39))])
        xs = -120.0 + 0.25 * np.arange(44)
        zs = -250.0 + 40250.0 * np.linspace(0.0, 1.0, 24) ** 1.6
    else:                                    # M2: 269 cells in x for the wide footprints
        ys = 10.0 + 0.5 * np.arange(8)
        xs = 100.0 + np.concatenate([[0.0], np.cumsum(0.2 + 0.1 * rng.random(269))])
        zs = np.array([-100.0, 300.0, 1200.0, 3500.0, 9000.0, 30000.0])
    wet, hyd = _fields(ys.size, xs.size, zs.size, zs, 11 if name == 'M1' else 12)
    return ys, xs, zs, wet, hyd


@pytest.fixture(scope='module')
def models():
    """{(name, dtype): (Cube on the device - y passed DESCENDING -, (ys, xs, zs, wet, hydro) ascending, in the cube's dtype)}"""
    import raider_amd as R
    out = {}
    for name in ('M1', 'M2'):
        ys, xs, zs, wet, hyd = _model(name)
        for dtype in (np.float32, np.float64):
            w, h = wet.astype(dtype), hyd.astype(dtype)
            for f in (w, h):
                for ax in range(3):
                    a, b = np.moveaxis(f, ax, 0)[1:].astype(np.float64), np.moveaxis(f, ax, 0)[:-1].astype(np.float64)
                    assert (np.abs(a - b) >= 1e-3 * np.maximum(np.abs(a), np.abs(b))).all(), 'model cube: neighbouring nodes too close'
            cube = R.Cube(ys[::-1].copy(), xs, zs, np.ascontiguousarray(w[::-1]), np.ascontiguousarray(h[::-1]), order='yxz')
            out[name, dtype] = (cube, (ys, xs, zs, w, h))
    return out


def _at(axis, u):
    """axis coordinate at the (fractional) cell position u"""
    return np.interp(np.asarray(u, dtype=np.float64), np.arange(axis.size), axis)


# ---- the long-double reference ----------------------------------------------------------------------------------------------------
def _axis_cells(g, q):
    ok = (q >= g[0]) & (q <= g[-1])                                     # (a NaN coordinate compares False)
    qs = np.where(ok, q, g[0])
    i = np.clip(np.searchsorted(g, qs, side='right') - 1, 0, g.size - 2)   # g[i] <= v < g[i+1], last cell closed
    return np.where(ok, i, -1), qs, ok


class _Ref:
    """the trilinear interpolant of one model cube on the output grid (xpts, ypts, zpts), output order (z, y, x)"""

    def __init__(self, data, xpts, ypts, zpts):
        self.g = data[:3]
        self.f = data[3:]
        self.q = (np.asarray(ypts, dtype=np.float64), np.asarray(xpts, dtype=np.float64), np.asarray(zpts, dtype=np.float64))
        self.shape = (self.q[2].size, self.q[0].size, self.q[1].size)
        (self.cy, self.sy, self.oky), (self.cx, self.sx, self.okx), (self.cz, self.sz, self.okz) = (_axis_cells(g, q) for g, q in zip(self.g, self.q))
        self._ld = None

    def nan_mask(self):
        return ~(self.okz[:, None, None] & self.oky[None, :, None] & self.okx[None, None, :])

    def _tables(self):
        if self._ld is None:
            t = []
            for g, c, s in zip(self.g, (self.cy, self.cx, self.cz), (self.sy, self.sx, self.sz)):
                i = np.maximum(c, 0)
                t.append((s.astype(LD) - g[i].astype(LD)) / (g[i + 1].astype(LD) - g[i].astype(LD)))
            self._ld = (t, [f.astype(LD) for f in self.f])
        return self._ld

    def at(self, kz, jy, jx):
        """[(value, A) for wet, hydro] at the output elements (kz, jy, jx): index arrays that broadcast against each other"""
        (ty, tx, tz), fields = self._tables()
        ty, tx, tz = ty[jy], tx[jx], tz[kz]
        iy, ix, iz = np.maximum(self.cy, 0)[jy], np.maximum(self.cx, 0)[jx], np.maximum(self.cz, 0)[kz]
        ok = self.oky[jy] & self.okx[jx] & self.okz[kz]
        one = LD(1)
        a = [(one - ty) * (one - tx), (one - ty) * tx, ty * (one - tx), ty * tx]
        k = [a[n >> 1] * (tz if n & 1 else one - tz) for n in range(8)]
        out = []
        for f in fields:
            s, A = LD(0), LD(0)
            for n, (dy, dx, dz) in enumerate(itertools.product((0, 1), repeat=3)):      # lexicographic (y, x, z)
                v = f[iy + dy, ix + dx, iz + dz]
                s = s + v * k[n]
                A = A + np.abs(v) * k[n]
            out.append((np.where(ok, s, LD('nan')), np.where(ok, A, LD(0))))
        return out

    def exact(self, kz, jy, jx):
        """one output element in exact rationals: [(value, A) for wet, hydro], None outside"""
        F = fractions.Fraction
        if not (self.oky[jy] and self.okx[jx] and self.okz[kz]):
            return None
        c = (int(self.cy[jy]), int(self.cx[jx]), int(self.cz[kz]))
        t = [(F(float(s[j])) - F(float(g[i]))) / (F(float(g[i + 1])) - F(float(g[i]))) for g, s, j, i in zip(self.g, (self.sy, self.sx, self.sz), (jy, jx, kz), c)]
        out = []
        for f in self.f:
            s, A = F(0), F(0)
            for dy, dx, dz in itertools.product((0, 1), repeat=3):
                kk = (t[0] if dy else 1 - t[0]) * (t[1] if dx else 1 - t[1]) * (t[2] if dz else 1 - t[2])
                v = F(float(f[c[0] + dy, c[1] + dx, c[2] + dz]))
                s += v * kk
                A += abs(v) * kk
            out.append((s, A))
        return out


def _selections(shape, full):
    """the index sets the reference is evaluated on: everything, or a fixed stride sample of >= 2e5 elements plus every tile-edge
    column (x % 64 in {0, 63}, the last) and row (y % 4 in {0, 3}, the last) at every height"""
    nz, ny, nx = shape
    kz, jy, jx = np.arange(nz)[:, None, None], np.arange(ny)[None, :, None], np.arange(nx)[None, None, :]
    n = nz * ny * nx
    if full or n <= 300000:
        return [(kz, jy, jx)]
    stride = max(1, n // 200000)
    while math.gcd(stride, 2 * nx * ny) != 1:        # (odd and coprime to the row / plane length: every lane and tile row gets hit)
        stride -= 1
    k, j, i = np.unravel_index(np.arange(0, n, stride), shape)
    cols = np.array(sorted({c for c in range(nx) if c % 64 in (0, 63)} | {nx - 1}))
    rows = np.array(sorted({r for r in range(ny) if r % 4 in (0, 3)} | {ny - 1}))
    return [(k, j, i), (kz, jy, cols[None, None, :]), (kz, rows[None, :, None], jx)]


def _check_against_reference(ref, got, full):
    """NaN mask identical and |gpu - ref| <= BOUND eps A; returns the largest |gpu - ref| / (eps A) seen"""
    worst = 0.0
    if np.finfo(LD).nmant >= 63:
        for sel in _selections(ref.shape, full):
            for g, (r, A) in zip(got, ref.at(*sel)):
                gs = g[sel]
                nan = np.isnan(r)
                assert np.array_equal(np.isnan(gs), nan), 'NaN mask differs from the reference'
                d, lim = np.abs(gs[~nan].astype(LD) - r[~nan]), LD(EPS) * A[~nan]
                if d.size:
                    worst = max(worst, float(np.max(d / lim)))
                    assert (d <= BOUND * lim).all(), f'|gpu - ref| reaches {float(np.max(d / lim)):.3g} eps A (bound {BOUND})'
    else:                                            # no 64-bit mantissa: exact rationals on a fixed 2000-point sample, the same bound
        F = fractions.Fraction
        n = ref.shape[0] * ref.shape[1] * ref.shape[2]
        for flat in np.linspace(0, n - 1, min(n, 2000)).astype(np.int64):
            kz, jy, jx = (int(v) for v in np.unravel_index(flat, ref.shape))
            e = ref.exact(kz, jy, jx)
            for g, ra in zip(got, e or (None, None)):
                if ra is None:
                    assert np.isnan(g[kz, jy, jx]), 'NaN mask differs from the reference'
                    continue
                assert not np.isnan(g[kz, jy, jx]), 'NaN mask differs from the reference'
                d, lim = abs(F(float(g[kz, jy, jx])) - ra[0]), F(EPS) * ra[1]
                worst = max(worst, float(d / lim))
                assert d <= BOUND * lim, f'|gpu - ref| reaches {float(d / lim):.3g} eps A (bound {BOUND})'
    return worst


# ---- the schedule model -----------------------------------------------------------------------------------------------------------
def _extent(c, width):
    """per tile of `width` consecutive output rows / columns: (smallest, largest) cell of its in-range entries, largest = -1 if none"""
    nt = -(-c.size // width)
    pad = np.full(nt * width, -1, dtype=np.int64)
    pad[:c.size] = c
    pad = pad.reshape(nt, width)
    return np.where(pad >= 0, pad, np.iinfo(np.int64).max).min(axis=1), pad.max(axis=1), (pad >= 0).sum(axis=1)


class _Sched:
    """build_cube_impl's launch arithmetic and build_cube_kernel's per-tile rule, restated"""

    def __init__(self, K, cus, dtype, ref):
        nz, ny, nx = ref.shape
        self.tiles_x, self.tiles_y = -(-nx // 64), -(-ny // 4)
        self.ntile = self.tiles_x * self.tiles_y
        nchunks = min(nz, max(1, -(-8 * cus // self.ntile)))
        nchunks = max(nchunks, -(-nz // K['BUILD_ZCHUNK_MAX']))
        self.zchunk = -(-nz // nchunks)
        self.nchunks = -(-nz // self.zchunk)
        self.gridx = max(1, min(self.ntile, 16 * cus))
        self.nzc = [min(self.zchunk, nz - c * self.zchunk) for c in range(self.nchunks)]
        self.stage_elems = K['BUILD_STAGE_BYTES'] // (2 * np.dtype(dtype).itemsize)
        self.ncol_max = K['BUILD_NCOL_MAX']
        self.UD = 4 if np.dtype(dtype).itemsize == 4 else 2
        ylo, yhi, yn = _extent(ref.cy, 4)
        xlo, xhi, xn = _extent(ref.cx, 64)
        some = (yhi >= 0)[:, None] & (xhi >= 0)[None, :]
        ey, ex = np.where(yhi >= 0, yhi - ylo + 2, 0), np.where(xhi >= 0, xhi - xlo + 2, 0)
        self.ncol = np.where(some, ey[:, None] * ex[None, :], 0).ravel()              # tile t = ty * tiles_x + tx, as the kernel counts
        self.inside = (yn[:, None] * xn[None, :]).ravel()                             # in-range nodes per tile
        self.nodes = (np.minimum(4, ny - 4 * np.arange(self.tiles_y))[:, None] * np.minimum(64, nx - 64 * np.arange(self.tiles_x))[None, :]).ravel()
        self.staged = (self.ncol > 0) & (self.ncol <= self.ncol_max) & (2 * self.ncol <= self.stage_elems)
        self.cz = ref.cz

    def U(self, t, nzc):
        return max(1, min(nzc, self.stage_elems // (2 * int(self.ncol[t])))) if self.staged[t] else 1

    def rounds(self, t, nzc):
        """heights per staging round of tile t in a chunk of nzc heights"""
        U = self.U(t, nzc)
        return [min(U, nzc - kb) for kb in range(0, nzc, U)]

    def batches(self, nzc):
        """heights stored per direct batch of a chunk of nzc heights (the loads of the tail are clamped, its stores cut)"""
        return [min(self.UD, nzc - kb) for kb in range(0, nzc, self.UD)]

    def trips(self, b):
        """the tiles workgroup b takes, in order"""
        return list(range(b, self.ntile, self.gridx))

    def chunk_cells(self, c):
        return self.cz[c * self.zchunk:c * self.zchunk + self.nzc[c]]


# ---- one build, checked -----------------------------------------------------------------------------------------------------------
def _run(model, xpts, ypts, zpts, label, full=False):
    """build_cube on the device, checked in full against Cube.interp (bit for bit) and the NaN mask / has_nan of the reference, and
    against the long-double reference (in full, or on the sample of _selections); returns (wet, hydro)"""
    cube, data = model
    ref = _Ref(data, xpts, ypts, zpts)
    w, h, flag = cube.build_cube(xpts, ypts, zpts, want_nan=True)
    nz, ny, nx = ref.shape
    assert w.shape == h.shape == ref.shape
    nan = ref.nan_mask()
    assert np.array_equal(np.isnan(w), nan) and np.array_equal(np.isnan(h), nan), f'{label}: NaN mask differs from the reference'
    assert flag is not None and flag == bool(nan.any()), f'{label}: has_nan = {flag}, the reference says {bool(nan.any())}'
    pts = np.empty(ref.shape + (3,))
    pts[..., 0] = ref.q[0][None, :, None]; pts[..., 1] = ref.q[1][None, None, :]; pts[..., 2] = ref.q[2][:, None, None]
    iw, ih = cube.interp(pts)
    assert np.array_equal(w, iw, equal_nan=True) and np.array_equal(h, ih, equal_nan=True), f'{label}: not the bits of Cube.interp'
    worst = _check_against_reference(ref, (w, h), full)
    print(f'[zenith-schedules] {label}: {nx} x {ny} x {nz}, max |gpu - ref| / (eps A) = {worst:.3f}')
    return w, h


def _name(dtype):
    return 'f32' if np.dtype(dtype).itemsize == 4 else 'f64'


def _heights(zs, n, seed, dirty=False):
    """n heights in random order: every z node (the first and last among them), the rest spread over all z cells (many per cell).
    dirty: heights below and above the axis between inside ones, one exactly at z_hi and one a hair above it"""
    rng = np.random.default_rng(seed)
    h = np.concatenate([zs, _at(zs, rng.uniform(0.0, zs.size - 1.0, n - zs.size))])
    rng.shuffle(h)
    if dirty:
        h[1::9] = zs[0] - 10.0 - rng.uniform(0, 500, h[1::9].size)
        h[4::9] = zs[-1] + 5.0 + rng.uniform(0, 500, h[4::9].size)
        h[7] = zs[-1]
        h[8] = np.nextafter(zs[-1], np.inf)
    return h


# ---- the cases --------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_one_chunk_staged_single_round(models, K, cus, dtype):
    """case 1: >= 8 CUs tiles, so ONE chunk of 11 heights; every tile staged in a single round; a 70 x 16 block of the same axis
    values built as its own small grid (one height per chunk) gives the same bits"""
    model = models['M1', dtype]
    ys, xs, zs = model[1][:3]
    nx, ny = 70, 4 * (-(-8 * cus // 2)) + 3
    xpts = _at(xs, 5.3 + 0.1 * np.arange(nx))
    ypts = _at(ys, np.linspace(38.6, 0.4, ny))
    zpts = _at(zs, 0.5 + 2.1 * np.arange(11))
    S = _Sched(K, cus, dtype, _Ref(model[1], xpts, ypts, zpts))
    assert S.nchunks == 1 and S.zchunk == 11, f'the heuristics no longer give one chunk here: {S.nchunks} chunks of {S.zchunk}'
    assert S.staged.all() and S.tiles_x == 2, 'not every tile is staged'
    assert all(S.rounds(t, 11) == [11] for t in range(S.ntile)), 'a tile needs more than one staging round'
    w, h = _run(model, xpts, ypts, zpts, f'case1-{_name(dtype)}')
    assert not np.isnan(w).any()
    r0 = 4 * (ny // 8) + 1                                       # (not on a tile boundary of the large grid)
    sub = _Sched(K, cus, dtype, _Ref(model[1], xpts, ypts[r0:r0 + 16], zpts))
    assert sub.zchunk == 1 and sub.nchunks == 11, 'the small grid no longer runs one height per chunk'
    sw, sh = _run(model, xpts, ypts[r0:r0 + 16], zpts, f'case1-sub-{_name(dtype)}', full=True)
    assert np.array_equal(sw, w[:, r0:r0 + 16]) and np.array_equal(sh, h[:, r0:r0 + 16])


def _multi_round_grid(model, cus, dirty):
    ys, xs, zs = model[1][:3]
    if not dirty:                                                # 72 x 5 nodes: a full tile of 4 rows x 64 lanes and three ragged ones
        xpts = _at(xs, 3.1 + 0.2 * np.arange(72))
        ypts = _at(ys, 1.3 + 3.7 * np.arange(5))
    else:
        # tile column 0: 32 nodes west of the cube, the first x node, 31 nodes inside (one of them NaN); column 1 (8 lanes) ends on the last x node
        xpts = np.concatenate([xs[0] - 0.5 - 0.01 * np.arange(32)[::-1], [xs[0]], _at(xs, 0.4 * np.arange(1, 32)), _at(xs, 43.0 - 0.2 * np.arange(8)[::-1])])
        xpts[40] = np.nan
        xpts[-1] = xs[-1]
        # tile row 0: the first y node and three rows 3.7 cells apart; row 1: north of the cube, the last y node, NaN, north; row 2: north
        ypts = np.concatenate([[ys[0]], _at(ys, 3.7 * np.arange(1, 4)), [ys[-1] + 0.3, ys[-1], np.nan, ys[-1] + 0.7], [ys[-1] + 1.0]])
    ntile = -(-xpts.size // 64) * -(-ypts.size // 4)
    nz = 13 * -(-8 * cus // ntile) - 6                            # chunks of 13 heights, the last one of 7
    return xpts, ypts, _heights(zs, nz, 21, dirty)


def _assert_multi_round(S, t):
    assert S.zchunk == 13, f'the heuristics no longer give chunks of 13 heights here: {S.zchunk}'
    r = S.rounds(t, S.zchunk)
    assert S.staged[t] and len(r) >= 2 and r[-1] < r[0], f'tile {t}: no multi-round staging with a partial last round (rounds {r}, footprint {S.ncol[t]})'
    assert S.zchunk > S.U(t, S.zchunk) and S.zchunk % S.U(t, S.zchunk) != 0
    if S.UD == 2:
        assert len(r) >= 3, f'f64: fewer than three rounds ({r})'
    assert 0 < S.nzc[-1] < S.zchunk, 'no shorter last chunk'


@DTYPES
def test_multi_round_staging_with_partial_last_round(models, K, cus, dtype):
    """case 2: a footprint just under BUILD_NCOL_MAX columns and chunks of 13 heights: rounds 5 + 5 + 3 (f64) / 11 + 2 (f32); heights
    that repeat a z cell, sit on z nodes, the first and last z node; a ragged tile next to it stages its chunk in one round"""
    model = models['M1', dtype]
    xpts, ypts, zpts = _multi_round_grid(model, cus, False)
    ref = _Ref(model[1], xpts, ypts, zpts)
    S = _Sched(K, cus, dtype, ref)
    _assert_multi_round(S, 0)
    assert S.ncol[0] > S.ncol_max // 2 and S.nodes[0] == 256 and S.inside[0] == 256
    assert any(len(S.rounds(t, S.zchunk)) == 1 for t in range(S.ntile) if S.staged[t]), 'no single-round tile in the same launch'
    assert any(np.unique(S.chunk_cells(c)).size < S.nzc[c] for c in range(S.nchunks)), 'no chunk repeats a z cell'
    zs = model[1][2]
    assert np.isin(zs, zpts).all()
    w, _ = _run(model, xpts, ypts, zpts, f'case2-{_name(dtype)}')
    assert not np.isnan(w).any()


def _direct_grid(model, cus, dirty):
    ys, xs, zs = model[1][:3]
    if not dirty:                                                # 64 nodes over the whole x range, 4 rows over 6.6 cells, a fifth row
        xpts = _at(xs, np.linspace(0.0, 43.0, 64))
        ypts = _at(ys, 2.2 + 2.2 * np.arange(5))
    else:
        # 16 nodes west of the cube, the first x node, 46 over the range (one NaN), the last x node: one part-outside tile column
        xpts = np.concatenate([xs[0] - 0.5 - 0.01 * np.arange(16)[::-1], [xs[0]], _at(xs, np.linspace(0.9, 42.3, 46)), [xs[-1]]])
        xpts[30] = np.nan
        ypts = np.concatenate([[ys[0]], _at(ys, 2.2 * np.arange(1, 4)), [ys[-1] + 0.3, ys[-1], np.nan, ys[-1] + 0.7], [ys[-1] + 1.0]])
    ntile = -(-xpts.size // 64) * -(-ypts.size // 4)
    nz = 7 * -(-8 * cus // ntile) - 2                             # chunks of 7 heights, the last one of 5
    return xpts, ypts, _heights(zs, nz, 22, dirty)


def _assert_direct(S, t):
    assert S.zchunk == 7, f'the heuristics no longer give chunks of 7 heights here: {S.zchunk}'
    assert not S.staged[t] and S.ncol[t] > S.ncol_max, f'tile {t} is not on the direct path (footprint {S.ncol[t]})'
    assert S.batches(7) == ([4, 3] if S.UD == 4 else [2, 2, 2, 1]), f'batches {S.batches(7)}'
    assert S.nzc[-1] == 5


@DTYPES
def test_direct_path_with_batch_tail(models, K, cus, dtype):
    """case 3: a footprint of more than BUILD_NCOL_MAX columns, chunks of 7 heights: direct batches 4 + 3 (f32) / 2 + 2 + 2 + 1 (f64);
    each row of the tile built alone - a footprint of two cube rows, which the model says is staged - gives the same bits"""
    model = models['M1', dtype]
    xpts, ypts, zpts = _direct_grid(model, cus, False)
    S = _Sched(K, cus, dtype, _Ref(model[1], xpts, ypts, zpts))
    _assert_direct(S, 0)
    assert S.nodes[0] == 256 and S.inside[0] == 256
    w, h = _run(model, xpts, ypts, zpts, f'case3-{_name(dtype)}')
    assert not np.isnan(w).any()
    for j in range(4):
        row = _Sched(K, cus, dtype, _Ref(model[1], xpts, ypts[j:j + 1], zpts))
        assert row.ntile == 1 and row.staged[0], 'a single row is no longer staged'
        rw, rh, _ = model[0].build_cube(xpts, ypts[j:j + 1], zpts, want_nan=True)
        assert np.array_equal(rw[:, 0], w[:, j]) and np.array_equal(rh[:, 0], h[:, j]), f'row {j}: staged and direct differ'


@DTYPES
def test_second_tile_of_a_workgroup_staged(models, K, cus, dtype):
    """case 4: more tiles than workgroups: the grid-stride loop's second trip re-uses the staging area"""
    model = models['M1', dtype]
    ys, xs, zs = model[1][:3]
    nx, ny = 33, 4 * (16 * cus + 37) + 1
    xpts = _at(xs, 10.0 + 0.37 * np.arange(nx))
    ypts = _at(ys, np.linspace(0.2, 38.8, ny))
    zpts = _at(zs, [1.5, 7.25])
    S = _Sched(K, cus, dtype, _Ref(model[1], xpts, ypts, zpts))
    assert S.ntile > S.gridx and len(S.trips(0)) == 2, f'no workgroup takes a second tile: {S.ntile} tiles, {S.gridx} workgroups'
    assert S.nchunks == 1 and S.staged.all()
    w, _ = _run(model, xpts, ypts, zpts, f'case4-{_name(dtype)}', full=True)
    assert not np.isnan(w).any()


@DTYPES
def test_successive_tiles_alternate_staged_direct_staged(models, K, cus, dtype):
    """case 5: three tile columns - 64 nodes within two cells (staged), 64 nodes across 264 cells (direct), 17 fine nodes (staged) - and
    more than twice as many tiles as workgroups: since gridDim.x is no multiple of 3 a workgroup's three trips run staged -> direct ->
    staged.  (Three trips take 4 (2 x 16 CUs / 3 + 11) + 2 rows; with half as many no workgroup takes a third tile.)"""
    model = models['M2', dtype]
    ys, xs, zs = model[1][:3]
    ny = 4 * ((2 * 16 * cus) // 3 + 11) + 2
    xpts = np.concatenate([_at(xs, 100.0 + np.linspace(0.05, 1.95, 64)), _at(xs, np.linspace(2.5, 266.5, 64)), _at(xs, 200.0 + 0.11 * np.arange(17))])
    ypts = _at(ys, np.linspace(2.2, 3.9, ny))
    zpts = _at(zs, [0.4, 3.6])
    S = _Sched(K, cus, dtype, _Ref(model[1], xpts, ypts, zpts))
    assert S.tiles_x == 3 and S.gridx % 3 != 0 and S.ntile > 2 * S.gridx, f'{S.ntile} tiles, {S.gridx} workgroups'
    assert S.nchunks == 1 and S.zchunk == 2
    chains = [[bool(S.staged[t]) for t in S.trips(b)] for b in range(S.gridx)]
    assert [True, False, True] in chains, 'no workgroup runs staged -> direct -> staged'
    assert any(c[:2] == [False, True] for c in chains), 'no workgroup runs direct -> staged'
    assert (S.ncol[1::3] > S.ncol_max).all() and S.cz[0] != S.cz[1]
    w, _ = _run(model, xpts, ypts, zpts, f'case5-{_name(dtype)}')
    assert not np.isnan(w).any()


def _assert_dirty(S, ref, t):
    assert 0 < S.inside[t] < S.nodes[t], f'tile {t} is not partly outside the cube'
    assert ((S.inside == 0) & (S.ncol == 0)).any(), 'no tile wholly outside the cube'
    mixed = [c for c in range(S.nchunks) if (S.chunk_cells(c) < 0).any() and (S.chunk_cells(c) >= 0).any()]
    assert mixed, 'no chunk mixes heights inside and outside the z axis'
    z, zs = ref.q[2], ref.g[2]
    assert any((z[c * S.zchunk:c * S.zchunk + S.nzc[c]] < zs[0]).any() and (z[c * S.zchunk:c * S.zchunk + S.nzc[c]] > zs[-1]).any() for c in mixed)
    assert (z == zs[-1]).any() and (z == np.nextafter(zs[-1], np.inf)).any()
    assert np.isnan(ref.q[0]).sum() == 1 and np.isnan(ref.q[1]).sum() == 1
    for g, q in zip(ref.g[:2], ref.q[:2]):
        assert (q == g[0]).any() and (q == g[-1]).any()
    assert (ref.q[0] > ref.g[0][-1]).any() and (ref.q[1] < ref.g[1][0]).any()


@DTYPES
def test_dirty_waves_multi_round_staging(models, K, cus, dtype):
    """case 6, staged: the grid of case 2 with nodes west and north of the cube (a tile half outside, tiles wholly outside), a NaN in
    xpts and in ypts, nodes exactly on the first / last x and y node, heights below and above the z axis between inside ones, one
    exactly at z_hi and one a hair above: the guarded instantiation, the same rounds"""
    model = models['M1', dtype]
    xpts, ypts, zpts = _multi_round_grid(model, cus, True)
    ref = _Ref(model[1], xpts, ypts, zpts)
    S = _Sched(K, cus, dtype, ref)
    _assert_multi_round(S, 0)
    _assert_dirty(S, ref, 0)
    w, _ = _run(model, xpts, ypts, zpts, f'case6-staged-{_name(dtype)}')
    assert np.isnan(w).any() and np.isfinite(w).any()


@DTYPES
def test_dirty_waves_direct_path(models, K, cus, dtype):
    """case 6, direct: the grid of case 3 with the same additions"""
    model = models['M1', dtype]
    xpts, ypts, zpts = _direct_grid(model, cus, True)
    ref = _Ref(model[1], xpts, ypts, zpts)
    S = _Sched(K, cus, dtype, ref)
    _assert_direct(S, 0)
    _assert_dirty(S, ref, 0)
    w, _ = _run(model, xpts, ypts, zpts, f'case6-direct-{_name(dtype)}')
    assert np.isnan(w).any() and np.isfinite(w).any()


@DTYPES
def test_ragged_shapes(models, K, cus, dtype):
    """case 7: grids smaller than a tile, one lane or one row beyond it, on a fine (staged) and a coarse (direct) spacing, 5 heights"""
    model = models['M1', dtype]
    ys, xs, zs = model[1][:3]
    zpts = _at(zs, [0.2, 5.5, 5.7, 11.0, 22.9])
    paths = set()
    for nx, ny in ((1, 1), (63, 5), (65, 1), (1, 9)):
        for kind in ('fine', 'coarse'):
            if kind == 'fine':
                xpts, ypts = _at(xs, 5.2 + 0.07 * np.arange(nx)), _at(ys, 3.1 + 0.3 * np.arange(ny))
            else:
                xpts, ypts = _at(xs, np.linspace(0.3, 42.7, nx)), _at(ys, np.linspace(38.5, 0.5, ny))
            S = _Sched(K, cus, dtype, _Ref(model[1], xpts, ypts, zpts))
            assert S.zchunk == 1 and S.ntile == -(-nx // 64) * -(-ny // 4)
            paths |= {bool(s) for s in S.staged}
            w, _ = _run(model, xpts, ypts, zpts, f'case7-{nx}x{ny}-{kind}-{_name(dtype)}', full=True)
            assert w.shape == (5, ny, nx) and not np.isnan(w).any()
    assert paths == {True, False}, 'the ragged grids no longer reach both the staged and the direct path'
