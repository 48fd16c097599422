"""Both zero-Doppler kernels of raider_amd/csrc/orbit_kernels.h (orbit_los_fast_kernel up to ORBIT_LDS_MAX_SV state vectors,
orbit_los_kernel beyond) and the solve inside aztime_blend_kernel, pinned on the extended-precision restatement of the algorithm
they state (tests/orbit_anchor.py: solve_ld).  isce3 is absent: what is pinned is the algorithm as written, not parity with isce3.

Who decides what:
* `clear` targets: the reference's stopping rule is at least 1e-3 (relative) away from a tie at every iteration.  A float64
  evaluation then stops at the same iteration, and is held to `tol` = 8 x the distance of the float64 oracle from the reference on
  that case (ORACLE_DIST, measured by the CPU self-check below), never below 4 ulp of the quantity.
* `ambiguous` targets (the rest, <= 0.5 % of a case): one iteration more or fewer is legitimate; they must be finite where the
  reference is and agree to 0.2 x threshold in t (the contraction of this Newton step), propagated to range and look vector.
* `on_end` targets: the reference's root lies within tol of st[0] or st[-1] (the two roots placed exactly on the end nodes).  The
  in-span rule compares a float64 t that carries an error of up to tol with the end: NaN and a value within tol are both right.

The CPU self-checks (unmarked) run without a GPU; the GPU tests are marked one by one."""
import datetime as dt
import functools
import time

import numpy as np
import pytest

from oracle import raider_oracle as O
from tests import orbit_anchor as A

LD = np.longdouble
THRESHOLD = 1.0e-7
N_TARGETS = 4096
C_LIGHT = LD(299792458)
T0_SCENE = 603.7                                  # s on the orbits' clock at which the sensor stands beside the scene of the tick tests

# name: (state vectors, nominal spacing s, jitter s, seed of the targets, time at which the sensor stands beside the tick scene)
CASES = {
    'uniform': (121, 10.0, 0.0, 11, T0_SCENE),
    'jittered': (121, 10.0, 3.0, 12, T0_SCENE),
    'four': (4, 10.0, 0.0, 13, 13.0),
    'edge320': (320, 4.0, 0.0, 14, 570.0),
    'edge321': (321, 4.0, 0.0, 14, 570.0),               # the same first 320 vectors and the same targets
    'long': (401, 3.0, 0.0, 15, 540.0),
    'jittered-long': (330, 4.0, 1.5, 16, 600.0),
}
# max distance of the float64 oracle (O.orbit_look_vectors) from solve_ld on the clear, valid targets of each case: (t s, range m,
# look vector).  Measured by test_oracle_stays_within_the_stored_distances, stored rounded up; the GPU tolerance is 8 x these.
ORACLE_DIST = {
    'uniform': (1.7e-11, 4.9e-09, 1.1e-13),
    'jittered': (2.7e-11, 5.2e-09, 1.7e-13),
    'four': (2.0e-11, 5.3e-09, 1.3e-13),
    'edge320': (3.1e-11, 3.0e-09, 2.2e-13),
    'edge321': (3.0e-11, 3.1e-09, 2.7e-13),
    'long': (4.6e-11, 4.1e-09, 3.7e-13),
    'jittered-long': (2.2e-10, 2.5e-08, 1.5e-12),
}
AMBIGUOUS_CAP = 0.005
EPOCH = dt.datetime(2021, 1, 1, 6, 47, 0)         # that clock's zero: acquisitions at 06:57:03, three minutes before the 07:00 model


def _orbit_arrays(name):
    nsv, step, jitter, _, t0 = CASES[name]
    st = step * np.arange(nsv)
    if jitter:
        st = np.sort(st + np.random.default_rng(nsv).uniform(-jitter, jitter, nsv))
    sp, sv = A.kepler_orbit(st, t0, wobble_period=5.0 * step)
    return st, sp, sv


def _finite(x):
    return np.isfinite(np.asarray(x, np.float64))


@functools.lru_cache(maxsize=None)
def case(name, threshold=THRESHOLD):
    """orbit, targets and reference of one case (computed once, never modified)"""
    st, sp, sv = _orbit_arrays(name)
    gen = _orbit_arrays('edge320') if name == 'edge321' else (st, sp, sv)
    xyz, roots, kind = A.case_targets(*gen, seed=CASES[name][3], n_total=N_TARGETS)
    ref = A.solve_ld(st, sp, sv, xyz, threshold=threshold)
    sub = np.ones(N_TARGETS, bool)
    if not A.EXTENDED:                             # no 80-bit long double here: `decimal` on a subsample, and say so
        sub[400:] = False
        sub |= kind == 4
        t, rg, los = A.solve_decimal(st, sp, sv, xyz[:400], threshold=threshold)
        ref = ref._replace(t=np.concatenate([t, ref.t[400:]]), rg=np.concatenate([rg, ref.rg[400:]]), los=np.concatenate([los, ref.los[400:]]))
        print(f'[{name}] NumPy long double has {np.finfo(LD).nmant} mantissa bits: reference = decimal (40 digits) on the first 400 targets only')
    valid = _finite(ref.t)
    quant = [float(np.nanmax(np.abs(np.asarray(q, np.float64)))) for q in (ref.t, ref.rg, ref.los)]
    tol = tuple(max(8.0 * d, 4.0 * float(np.spacing(q))) for d, q in zip(ORACLE_DIST[name], quant))
    inside = _inside(st, sp, sv, xyz, threshold)
    on_end = np.abs(inside) <= tol[0]
    clear = np.asarray(ref.margin >= 1e-3) & ~on_end & sub
    ambiguous = ~np.asarray(ref.margin >= 1e-3) & ~on_end & sub
    out = dict(name=name, st=st, sp=sp, sv=sv, xyz=xyz, roots=roots, kind=kind, ref=ref, valid=valid, tol=tol, on_end=on_end, clear=clear,
               ambiguous=ambiguous, threshold=threshold)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _inside(st, sp, sv, xyz, threshold):
    """distance of the reference's converged root from the nearer end of the span, positive inside (inf: not converged / NaN target)"""
    T = np.asarray(xyz, LD)
    t = np.full(T.shape[0], LD(0.5) * (LD(st[0]) + LD(st[-1])))
    done = np.zeros(T.shape[0], bool)
    for _ in range(30):
        pos, vel = A.hermite_ld(st, sp, sv, t)
        step = ((T - pos) * vel).sum(-1) / -(vel * vel).sum(-1)
        step = np.where(done, 0, step)
        t = t - step
        done |= np.abs(step) < LD(threshold)
    d = np.minimum(t - LD(st[0]), LD(st[-1]) - t)
    return np.where(done & np.isfinite(T).all(-1), d, np.inf).astype(np.float64)


def _distances(c, los, az, rg, where):
    ref = c['ref']
    if not where.any():
        return 0.0, 0.0, 0.0
    return (float(np.abs(az[where] - ref.t[where]).max()), float(np.abs(rg[where] - ref.rg[where]).max()),
            float(np.abs(los[where] - ref.los[where]).max()))


def check_against_reference(c, los, az, rg, label):
    """section 2b of the module's contract for one (case, solver output); returns the observed maxima on the clear targets"""
    ref, valid, clear, amb, on_end, tol, kind = (c[k] for k in ('ref', 'valid', 'clear', 'ambiguous', 'on_end', 'tol', 'kind'))
    fin = np.isfinite(az)
    assert np.array_equal(np.isfinite(rg), fin) and np.array_equal(np.isfinite(los).all(-1), fin) and np.array_equal(np.isfinite(los).any(-1), fin)
    # finite mask on the clear targets, both directions; the roots outside either end and the NaN targets are among them
    assert not (fin & ~valid & clear).any(), f'{label}: finite where the reference fails: {np.nonzero(fin & ~valid & clear)[0][:8]}'
    assert not (~fin & valid & clear).any(), f'{label}: NaN where the reference is valid: {np.nonzero(~fin & valid & clear)[0][:8]}'
    outside = (c['roots'] < c['st'][0] - 0.1) | (c['roots'] > c['st'][-1] + 0.1)
    assert outside.sum() >= 50 and not fin[outside | (kind == 4)].any()                # roots 0.3 to 5 s outside, NaN targets
    for q in np.nonzero(kind == 4)[0]:                                         # the neighbours of a NaN target are unaffected
        for nb in (q - 1, q + 1):
            assert on_end[nb] or fin[nb] == valid[nb]
    got = _distances(c, los, az, rg, clear & valid)
    print(f'{label}: clear {int((clear & valid).sum())} max |dt| {got[0]:.2e} s (tol {tol[0]:.2e}), |drg| {got[1]:.2e} m (tol {tol[1]:.2e}), '
          f'|dlos| {got[2]:.2e} (tol {tol[2]:.2e}); ambiguous {int(amb.sum())}, on an end {int(on_end.sum())}')
    assert got[0] <= tol[0] and got[1] <= tol[1] and got[2] <= tol[2], (label, got, tol)
    # ambiguous targets: finite where the reference is, within the contraction of one Newton step
    assert amb.mean() <= AMBIGUOUS_CAP
    w = amb & valid
    assert fin[w].all()
    if w.any():
        dt_max = 0.2 * c['threshold']
        speed2 = np.asarray((ref.vel * ref.vel).sum(-1), np.float64)[w]
        rgw = np.asarray(ref.rg, np.float64)[w]
        assert (np.abs(az[w] - ref.t[w]) <= dt_max + tol[0]).all()
        assert (np.abs(rg[w] - ref.rg[w]) <= tol[1] + speed2 / rgw * (c['threshold'] * dt_max + dt_max ** 2)).all()
        assert (np.abs(los[w] - ref.los[w]).max(-1) <= tol[2] + np.sqrt(speed2) * dt_max / rgw).all()
    # a root on an end node: NaN, or the value
    w = on_end & fin
    assert on_end.sum() <= 2 and (kind[on_end] == 1).all()
    if w.any():
        e = _distances(c, los, az, rg, w & valid)
        assert e[0] <= tol[0] and e[1] <= tol[1] and e[2] <= tol[2]
    # |los| = 1 to 2 ulp
    l = np.asarray(los[fin], LD)
    assert np.abs(np.sqrt((l * l).sum(-1)) - 1).max() <= 2 * np.finfo(np.float64).eps
    return got


# ---- CPU self-checks of the reference -------------------------------------------------------------------------------------------
def test_reference_meets_the_closed_form_of_a_circular_orbit():
    """solve_ld on the circular equatorial orbit of orbit_anchor: azimuth time lon / w, law-of-cosines range and the look vector,
    to the Hermite error documented there (2e-4 m; the bounds are those the oracle's restatement is held to)"""
    st, sp, sv = A.circular_orbit()
    T, t0, rg0, los0 = A.targets(np.random.default_rng(0))
    r = A.solve_ld(st, sp, sv, T)
    assert _finite(r.t).all() and (r.count <= 30).all()
    assert np.abs(r.t - t0).max() < 1e-6 and np.abs(r.rg - rg0).max() < 1e-3 and np.abs(r.los - los0).max() < 1e-8
    pos, vel = A.hermite_ld(st, sp, sv, st)                                    # the nodes themselves
    assert np.abs(pos - sp).max() < 1e-9 and np.abs(vel - sv).max() < 1e-12


def test_reference_against_decimal_arithmetic():
    """solve_ld against the same iteration in 40-digit decimal arithmetic on a subsample: 64-bit mantissa rounding, nothing more"""
    c = case('jittered')
    n = 400 if not A.EXTENDED else 48
    r = A.solve_ld(c['st'], c['sp'], c['sv'], c['xyz'][:n])
    t, rg, los = A.solve_decimal(c['st'], c['sp'], c['sv'], c['xyz'][:n])
    ok = _finite(r.t)
    assert np.array_equal(np.isfinite(t), ok) and ok.sum() > 0.8 * n
    lim = 1e-15 if A.EXTENDED else 1e-9
    assert np.abs(np.asarray(r.t, np.float64) - t)[ok].max() <= lim * 1e3 and np.abs(np.asarray(r.rg, np.float64) - rg)[ok].max() <= lim * 1e6
    assert np.abs(np.asarray(r.los, np.float64) - los)[ok].max() <= lim


def test_lla2ecef_ld_against_the_oracle():
    rng = np.random.default_rng(5)
    la, lo, h = rng.uniform(-89, 89, 500), rng.uniform(-180, 180, 500), rng.uniform(-400, 9000, 500)
    assert np.abs(A.lla2ecef_ld(la, lo, h) - np.stack(O.lla2ecef(la, lo, h), -1)).max() < 1e-8


@pytest.mark.parametrize('name', list(CASES))
def test_case_holds_what_it_must(name):
    """every case: a root on every node, >= 50 roots in the first and in the last interval and outside either end, two NaN targets;
    roots outside are NaN in the reference; ambiguous targets under the cap; iteration counts under the default cap"""
    c = case(name)
    st, roots, kind, ref, valid = (c[k] for k in ('st', 'roots', 'kind', 'ref', 'valid'))
    span = _orbit_arrays('edge320')[0] if name == 'edge321' else st
    assert np.array_equal(np.sort(roots[kind == 1]), span)
    inner = roots[kind == 2]
    assert ((inner > span[0]) & (inner < span[1])).sum() >= 50 and ((inner > span[-2]) & (inner < span[-1])).sum() >= 50
    outer = roots[kind == 3]
    assert ((span[0] - outer >= 0.3) & (span[0] - outer <= 5.0)).sum() >= 50 and ((outer - span[-1] >= 0.3) & (outer - span[-1] <= 5.0)).sum() >= 50
    assert (kind == 4).sum() == 2 and np.isnan(c['xyz'][kind == 4]).sum() == 2 and not valid[kind == 4].any()
    assert not valid[(kind == 3) & ((roots < st[0] - 0.1) | (roots > st[-1] + 0.1))].any()
    inside = (kind != 4) & (roots >= st[0]) & (roots <= st[-1]) & ~c['on_end']
    assert valid[inside].all()
    if A.EXTENDED:
        known = valid & (roots < span[-3]) if name == 'edge321' else valid     # (built on the 320-vector orbit: other windows at its end)
        assert np.abs(ref.t - roots)[known].max() < 1e-7                       # the reference finds the roots the targets were built from
    assert c['ambiguous'].mean() <= AMBIGUOUS_CAP and c['on_end'].sum() <= 2
    converged = ref.count[kind != 4]
    print(f'[{name}] iterations max {converged.max()}, ambiguous {int(c["ambiguous"].sum())} of {N_TARGETS}, on an end {int(c["on_end"].sum())}')
    assert converged.max() <= 30


@pytest.mark.parametrize('name', list(CASES))
def test_oracle_stays_within_the_stored_distances(name):
    """where ORACLE_DIST comes from: the float64 oracle against the reference on the clear, valid targets of the case"""
    c = case(name)
    los, az, rg = O.orbit_look_vectors(c['st'], c['sp'], c['sv'], c['xyz'])
    w = c['clear'] & c['valid']
    assert np.array_equal(np.isfinite(az)[c['clear']], c['valid'][c['clear']])
    got = _distances(c, los, az, rg, w)
    print(f'[{name}] oracle - reference: {got[0]:.3e} s, {got[1]:.3e} m, {got[2]:.3e}; stored {ORACLE_DIST[name]}')
    assert all(g <= s for g, s in zip(got, ORACLE_DIST[name]))
    if A.EXTENDED:
        assert all(s <= 1.25 * g for g, s in zip(got, ORACLE_DIST[name]))     # and the stored figures are not padded


@pytest.mark.parametrize('name', [n for n in CASES if n != 'four'])        # four vectors: one window, none to mistake it for
def test_a_window_one_node_off_is_visible(name):
    """solve_ld with the node window shifted down by one node moves t by >= 100 x the case's tol on at least half of the clear targets:
    the tolerance sees a wrong window with two orders to spare"""
    c = case(name)
    off = A.solve_ld(c['st'], c['sp'], c['sv'], c['xyz'], shift=1)
    w = c['clear'] & c['valid'] & _finite(off.t)
    moved = np.abs(np.asarray(off.t - c['ref'].t, np.float64))[w]
    print(f'[{name}] window off by one: median |dt| {np.median(moved):.2e} s = {np.median(moved) / c["tol"][0]:.0f} x tol')
    assert w.sum() > 0.9 * (c['clear'] & c['valid']).sum() and np.median(moved) >= 100.0 * c['tol'][0]


# ---- the scene of the tick tests -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tick_scene(name):
    """the 7 x 33 x 41 rotated scene of test_gpu_time_interp.py under a 121-vector orbit: reference ticks, and the voxels left out"""
    from tests.test_gpu_time_interp import NX, NY, NZ, _rotated
    ys, xs, zs = np.linspace(30, 31, NY), np.linspace(-118, -117, NX), np.linspace(0, 9000, NZ)
    lat2, lon2 = _rotated(ys, xs)
    st, sp, sv = _orbit_arrays(name) if name in CASES else _short_orbit()
    shape = (NZ, NY, NX)
    xyz = A.lla2ecef_ld(np.broadcast_to(lat2, shape), np.broadcast_to(lon2, shape), np.broadcast_to(zs[:, None, None], shape))
    ref = A.solve_ld(st, sp, sv, xyz.reshape(-1, 3), maxiter=100)
    ms = ((ref.t + ref.rg / C_LIGHT) * 1e3).reshape(shape)
    with np.errstate(invalid='ignore'):
        near = np.asarray(np.abs(ms - np.rint(ms)) < 1e-4)                    # within 1e-7 s, the solver's threshold, of a tick boundary
    tick = np.where(_finite(ms), np.floor(ms), -1).astype(np.int64)
    return dict(ys=ys, xs=xs, zs=zs, lat2=lat2, lon2=lon2, st=st, sp=sp, sv=sv, shape=shape, tick=tick, near=near, valid=_finite(ms),
                inside=_inside(st, sp, sv, xyz.reshape(-1, 3), THRESHOLD).reshape(shape))


def _short_orbit():
    """13 state vectors that end while the sensor passes the scene: zero Doppler exists for part of the voxels only"""
    st = 10.0 * np.arange(13)
    return (st,) + A.kepler_orbit(st, st[-1] + 13.0, wobble_period=50.0)


@pytest.mark.parametrize('name', ['uniform', 'jittered'])
def test_tick_scene_leaves_out_few_voxels(name):
    s = tick_scene(name)
    print(f'[{name}] tick scene: {int(s["near"].sum())} of {s["near"].size} voxels within 1e-4 ms of a tick boundary')
    assert s['valid'].all() and s['near'].mean() <= 0.002
    assert s['tick'].min() > 500_000 and s['tick'].max() < 700_000 and np.ptp(s['tick']) > 10_000          # 17 s across the scene, mid-orbit


def test_partial_scene_splits_cleanly():
    s = tick_scene('short')
    share = s['valid'].mean()
    print(f'[short] {share:.3f} of the voxels have a zero-Doppler time inside the orbit; nearest to the end {np.abs(s["inside"]).min():.2e} s')
    assert 0.1 <= share <= 0.9 and np.abs(s['inside']).min() > 1e-6


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def _kernel(nsv):
    from raider_amd import _lib as L
    return 'fast' if nsv <= L.ORBIT_LDS_MAX_SV else 'slow'


def _orbit(c, epoch=None):
    from raider_amd.orbits import Orbit
    return Orbit(list(c['st']), c['sp'], c['sv'], epoch=epoch)


_GPU = {}


def gpu_solve(name, threshold=THRESHOLD, maxiter=30):
    key = (name, threshold, maxiter)
    if key not in _GPU:
        c = case(name, threshold)
        t0 = time.perf_counter()
        _GPU[key] = _orbit(c).look_vectors(c['xyz'], threshold=threshold, maxiter=maxiter, return_geometry=True)
        print(f'[{name}] look_vectors: {1e3 * (time.perf_counter() - t0):.1f} ms')
        for a in _GPU[key]:
            a.setflags(write=False)
    return _GPU[key]


EXPECTED_KERNEL = {'uniform': 'fast', 'jittered': 'fast', 'four': 'fast', 'edge320': 'fast', 'edge321': 'slow', 'long': 'slow', 'jittered-long': 'slow'}


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(CASES))
def test_solver_against_the_reference(name):
    """2a / 2b: finite mask, t, range, look vector and norm of Orbit.look_vectors against solve_ld on every case"""
    c = case(name)
    assert _kernel(c['st'].size) == EXPECTED_KERNEL[name] and c['st'].size == CASES[name][0]
    if 'jittered' in name:
        assert np.ptp(np.diff(c['st'])) > CASES[name][2]                      # times the segment guess of the fast kernel is wrong for
    los, az, rg = gpu_solve(name)
    check_against_reference(c, los, az, rg, f'[{name}] GPU')


@pytest.mark.gpu
def test_fast_and_slow_kernel_on_the_same_targets():
    """The edge case: 320 vectors (LDS tables at their limit) and the same plus one (slow kernel) on the same targets.  The two orbits
    have different mid times, so their Newton iterates differ, and at the product's threshold each stops up to 0.25 x 1e-7 s from the
    root on its own side.  With threshold 1e-10 both stop within 2.5e-11 s of it: each is held to its reference at tol, and the two to
    each other at 2 tol wherever they interpolate through the same four nodes (roots before node 318; later ones sit in windows that
    the end of the shorter orbit clamps)."""
    thr = 1.0e-10
    a, b = case('edge320', thr), case('edge321', thr)
    assert _kernel(a['st'].size) == 'fast' and _kernel(b['st'].size) == 'slow' and np.array_equal(a['xyz'], b['xyz'], equal_nan=True)
    assert np.array_equal(a['st'], b['st'][:320]) and np.array_equal(a['sp'], b['sp'][:320]) and np.array_equal(a['sv'], b['sv'][:320])
    ga, gb = gpu_solve('edge320', thr), gpu_solve('edge321', thr)
    for c, g in ((a, ga), (b, gb)):
        ref, w = c['ref'], c['valid'] & ~c['on_end']
        assert np.isfinite(g[1])[w].all() and not np.isfinite(g[1])[~c['valid'] & ~c['on_end']].any()
        got = _distances(c, *g, w)
        print(f'[{c["name"]} threshold 1e-10] max |dt| {got[0]:.2e} s, |drg| {got[1]:.2e} m, |dlos| {got[2]:.2e}; tol {c["tol"]}')
        assert all(x <= t for x, t in zip(got, c['tol']))
    both = a['valid'] & b['valid'] & ~a['on_end'] & ~b['on_end'] & np.asarray(a['ref'].t < a['st'][318])
    assert both.sum() > 0.9 * N_TARGETS and (a['kind'][both] == 1).sum() >= 317 and ((a['kind'] == 2) & both).sum() >= 50
    d = (np.abs(ga[1] - gb[1])[both].max(), np.abs(ga[2] - gb[2])[both].max(), np.abs(ga[0] - gb[0])[both].max())
    print(f'[edge] fast - slow on {int(both.sum())} targets: {d[0]:.2e} s, {d[1]:.2e} m, {d[2]:.2e}')
    assert all(x <= 2.0 * max(ta, tb) for x, ta, tb in zip(d, a['tol'], b['tol']))


@pytest.mark.gpu
def test_iteration_cap():
    """maxiter = 11 on the uniform case: finite exactly where the reference converges within 11 evaluations"""
    c = case('uniform')
    want = c['valid'] & (c['ref'].count <= 11)
    decided = c['clear'] & (c['kind'] != 4)
    share = want[decided & c['valid']].mean()
    print(f'[uniform] maxiter 11: the reference converges on {share:.3f} of the valid targets')
    assert 0.1 <= share <= 0.9
    los, az, rg = gpu_solve('uniform', maxiter=11)
    assert np.array_equal(np.isfinite(az)[decided], want[decided])
    assert np.array_equal(np.isfinite(rg), np.isfinite(az)) and np.array_equal(np.isfinite(los).all(-1), np.isfinite(az))
    full = gpu_solve('uniform')
    w = decided & want
    assert all(np.array_equal(x[w], y[w]) for x, y in zip((los, az, rg), full))          # and the same bytes as under the default cap


def _bits(arrays):
    return [np.ascontiguousarray(a).view(np.uint64) for a in arrays]


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['uniform', 'long'])
def test_lane_and_launch_independence(name):
    """a target's bytes do not depend on the lane, the workgroup, the trip of the grid-stride loop or where the targets live"""
    import torch
    c = case(name)
    assert _kernel(c['st'].size) == EXPECTED_KERNEL[name]
    orb = _orbit(c)
    full = _bits(gpu_solve(name))
    for k in (1, 63, 64, 65, 257):
        part = _bits(orb.look_vectors(c['xyz'][:k], return_geometry=True))
        assert all(np.array_equal(p, f[:k]) for p, f in zip(part, full)), k
    dev = orb.look_vectors(torch.from_numpy(c['xyz'].copy()).to('cuda:0'), return_geometry=True)
    assert all(x.is_cuda for x in dev)
    assert all(np.array_equal(p, f) for p, f in zip(_bits([x.cpu().numpy() for x in dev]), full))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    reps = 8 * cus * 256 // N_TARGETS + 1                                      # more targets than one trip of the grid covers
    assert reps * N_TARGETS > 8 * cus * 256
    print(f'[{name}] {cus} CUs: {reps * N_TARGETS} targets in one call')
    big = _bits(orb.look_vectors(np.tile(c['xyz'], (reps, 1)), return_geometry=True))
    for p, f in zip(big, full):
        assert np.array_equal(p.reshape((reps,) + f.shape), np.broadcast_to(f, (reps,) + f.shape))


def _cubes(s):
    from raider_amd import Cube
    nz, ny, nx = s['shape']
    f = np.random.default_rng(16).uniform(0.5, 60.0, (3, 2, nz, ny, nx)).astype(np.float32)
    return [Cube(s['ys'], s['xs'], s['zs'], f[i, 0], f[i, 1], order='zyx') for i in range(3)]


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['uniform', 'jittered'])
def test_millisecond_ticks(name):
    """the fused kernel's time grid and the staged get_azimuth_time_grid both hit floor((t + range / c) 1e3) of the reference on every
    voxel that is not within 1e-4 ms of a tick boundary"""
    from raider_amd.s1_azimuth_timing import combine_cubes_azimuth_time, get_azimuth_time_grid
    from tests.test_gpu_time_interp import DATES
    s = tick_scene(name)
    assert s['near'].mean() <= 0.002
    orb = _orbit(s, EPOCH)
    _, _, grid = combine_cubes_azimuth_time(_cubes(s), None, DATES, s['lat2'], s['lon2'], orb, return_time_grid=True)
    sec = get_azimuth_time_grid(np.broadcast_to(s['lon2'], s['shape']), np.broadcast_to(s['lat2'], s['shape']),
                                np.broadcast_to(s['zs'][:, None, None], s['shape']), orb, as_datetime64=False)
    assert np.isfinite(grid).all() and np.isfinite(sec).all()
    fused = np.rint((grid + (DATES[0] - EPOCH).total_seconds()) * 1e3).astype(np.int64)
    staged = np.rint(sec * 1e3).astype(np.int64)
    keep = ~s['near']
    print(f'[{name}] ticks: {int((fused != s["tick"])[keep].sum())} fused and {int((staged != s["tick"])[keep].sum())} staged voxels off the reference, '
          f'{int(s["near"].sum())} of {keep.size} left out')
    assert np.array_equal(fused[keep], s['tick'][keep]) and np.array_equal(staged[keep], s['tick'][keep])
    assert (np.abs(fused - s['tick'])[~keep] <= 1).all() and (np.abs(staged - s['tick'])[~keep] <= 1).all()


@pytest.mark.gpu
def test_partial_failure():
    """an orbit that ends over the scene: the staged grid is NaN exactly on the reference's failing voxels, and the fused entry raises
    the reference's ValueError, flag bit 0 being set by some voxels and not by all"""
    from raider_amd.s1_azimuth_timing import combine_cubes_azimuth_time, get_azimuth_time_grid
    from tests.test_gpu_time_interp import DATES
    s = tick_scene('short')
    assert 0.1 <= s['valid'].mean() <= 0.9 and np.abs(s['inside']).min() > 1e-6
    orb = _orbit(s, dt.datetime(2021, 1, 1, 6, 55, 0))
    sec = get_azimuth_time_grid(np.broadcast_to(s['lon2'], s['shape']), np.broadcast_to(s['lat2'], s['shape']),
                                np.broadcast_to(s['zs'][:, None, None], s['shape']), orb, as_datetime64=False)
    assert np.array_equal(np.isfinite(sec), s['valid'])
    assert np.array_equal(np.rint(sec[s['valid'] & ~s['near']] * 1e3).astype(np.int64), s['tick'][s['valid'] & ~s['near']])
    with pytest.raises(ValueError, match='The Time Grid return nans meaning no orbit was downloaded.'):
        combine_cubes_azimuth_time(_cubes(s), None, DATES, s['lat2'], s['lon2'], orb)
