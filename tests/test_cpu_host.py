"""CPU: C-ABI library loads and exports every declared symbol; host-side logic; loud failure without a GPU;
the product never imports the oracle."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as g
    g.build()
    import raider_amd
    return raider_amd


def test_library_exports_every_header_symbol(built):
    from raider_amd import _lib
    hdr = (REPO / 'include' / 'raider_hip.h').read_text()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(rdr_[a-z0-9_]+)\s*\(', hdr))
    assert len(declared) >= 30
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in declared:
        assert hasattr(lib, name), f'{name} declared in include/raider_hip.h but not exported'
    bound = {s[0] for s in _lib.SYMBOLS}
    assert declared == bound, f'header vs ctypes table mismatch: {declared ^ bound}'
    assert _lib.load().rdr_version() >= 100


def test_binary_carries_the_hash_of_the_tree_it_was_built_from(built, tmp_path, monkeypatch):
    """build() compiles the sha256 of the sources into the library and rebuilds when the tree's differs (file times do not
    survive a copy to the GPU box); the digest is readable without dlopen-ing a possibly stale binary."""
    from raider_amd import _lib
    want = _lib.source_hash()
    assert len(want) == 16 and _lib.load().rdr_source_hash().decode() == want
    monkeypatch.setattr(_lib, '_lib', None)                       # force the read-the-file path
    assert _lib.binary_source_hash(_lib.LIB_PATH) == want
    assert _lib.binary_source_hash(tmp_path / 'missing.so') is None
    stale = tmp_path / 'stale.so'
    data = _lib.LIB_PATH.read_bytes()
    k = data.find(b'rdr-source-hash:')
    stale.write_bytes(data[:k + 16] + b'0' * 16 + data[k + 32:])
    assert _lib.binary_source_hash(stale) == '0' * 16             # what build() would see for a binary of another tree -> recompile
    assert {f.name for f in _lib.source_files()} >= {'raider_hip.hip', 'raider_kernels.h', 'cube_kernels.h', 'raider_hip.h'}


def test_rays_struct_layout_matches_header(built):
    from raider_amd import _lib
    # 8 + 4 + 4 + 8 + 8 + 8*8 + 8 + 8 + 4 + 4 + 8 (hts, round 3)
    assert ctypes.sizeof(_lib.RdrRays) == 128
    assert _lib.RdrRays.hts.offset == 120 and _lib.RdrRays.loc.offset == 112


def test_no_gpu_fails_loudly(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip('a GPU is present')
    from raider_amd import Context
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        Context(0)
    from scipy.interpolate import RegularGridInterpolator
    from raider_amd.delay import _build_cube
    ax = np.arange(3.0)
    rgi = RegularGridInterpolator((ax, ax, ax), np.zeros((3, 3, 3)))
    with pytest.raises(RuntimeError, match='no CPU fallback'):          # scipy objects are uploaded, never evaluated
        _build_cube(ax, ax, np.zeros(1), 4326, 4326, [rgi, rgi])


def test_missing_library_fails_loudly(built, monkeypatch, tmp_path):
    from raider_amd import _lib
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'LIB_PATH', tmp_path / 'nope.so')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        _lib.load()


def test_product_never_imports_oracle():
    for p in (REPO / 'raider_amd').rglob('*.py'):
        txt = p.read_text()
        assert 'oracle' not in re.sub(r'#.*', '', txt).replace('SURVEY', ''), f'{p} mentions the oracle'
    for p in (REPO / 'raider_amd' / 'csrc').iterdir():
        assert 'oracle' not in p.read_text(errors='ignore') or p.suffix == '.so'


def test_host_helpers_match_oracle():
    from oracle import raider_oracle as O
    from raider_amd.losreader import getZenithLookVecs, inc_hd_to_enu
    from raider_amd.utilFcns import cosd, ecef2enu, enu2ecef, sind
    rng = np.random.default_rng(1)
    inc = rng.uniform(0, 60, 50); hd = rng.uniform(-180, 180, 50); lat = rng.uniform(-80, 80, 50); lon = rng.uniform(-180, 180, 50)
    assert np.array_equal(inc_hd_to_enu(inc, hd), O.inc_hd_to_enu(inc, hd))
    enu = inc_hd_to_enu(inc, hd)
    e = enu2ecef(enu[:, 0], enu[:, 1], enu[:, 2], lat, lon, 0)
    np.testing.assert_allclose(e, O.enu2ecef(enu[:, 0], enu[:, 1], enu[:, 2], lat, lon, 0), rtol=0, atol=1e-16)
    np.testing.assert_allclose(ecef2enu(e, lat, lon, 0), enu, rtol=0, atol=1e-15)          # round trip (test/test_util.py:390-495)
    assert np.array_equal(getZenithLookVecs(lat, lon, 0), O.getZenithLookVecs(lat, lon, 0))
    assert cosd(60.0) == pytest.approx(0.5) and sind(30.0) == pytest.approx(0.5)
    with pytest.raises(ValueError):
        inc_hd_to_enu(np.array([-1.0]), np.array([0.0]))


def test_los_protocol():
    from raider_amd.losreader import Conventional, Raytracing, Zenith
    z = Zenith(); c = Conventional(inc=np.array([30.0])); r = Raytracing(inc=35.0, heading=-168.0)
    assert z.is_Zenith() and not z.is_Projected() and not z.ray_trace()
    assert c.is_Projected() and not c.is_Zenith()
    assert r.ray_trace() and not r.is_Zenith() and not r.is_Projected()
    import datetime
    with pytest.raises(ValueError):
        Raytracing('no_such_orbit.EOF', time=datetime.datetime(2020, 1, 1))      # get_sv: cannot parse (losreader.py:362-366)
    with pytest.raises(ValueError):
        Raytracing()
    with pytest.raises(RuntimeError):
        Raytracing(inc=1.0, look_dir='up')
    with pytest.raises(NotImplementedError):
        Conventional(los_convention='roipac')
    with pytest.raises(RuntimeError):
        Zenith().setPoints(None)
    z.setPoints(np.zeros((4, 3)))
    assert z._heights.shape == (4,)


def test_make_points_count(built):
    from raider_amd import _lib
    lib = _lib.load()
    for ml, st in ((1000., 5.), (20., 5.), (100., 5.), (12345.6, 15.0), (7.0, 2.0), (0.0, 1.0), (1.0, 0.3)):
        ref = int(ml // st) + (1 if ml % st != 0 else 0)            # makePoints.pyx:30-33
        assert lib.rdr_make_points_count(ml, st) == ref


def test_synthetic_matches_oracle_recipe():
    from oracle import raider_oracle as O
    from raider_amd.synthetic import synthetic_cube
    a = synthetic_cube(20, 24, 12, seed=3); b = O.synthetic_cube(20, 24, 12, seed=3)
    for k in a:
        assert np.array_equal(a[k], b[k])


def test_g9_orbit_readers(golden):
    """File readers against the reference's own readers run on its own fixtures (tests/golden/orbit_files = DATA copies
    of test/orbit_files/*; expected arrays from oracle/refharness/gen_golden.py g9)."""
    import datetime as dt
    from raider_amd import orbits
    g = golden('g9_orbit_readers')
    d = REPO / 'tests' / 'golden' / 'orbit_files'
    for tag, fn, reader in (('eof', 'S1_orbit_example.EOF', orbits.read_ESA_Orbit_file), ('txt', 'S1_sv_file.txt', orbits.read_txt_file)):
        svs = reader(str(d / fn))
        assert svs[0][0].isoformat() == str(g[f'{tag}_epoch'])
        assert np.array_equal([(t - svs[0][0]).total_seconds() for t in svs[0]], g[f'{tag}_t'])
        assert np.array_equal(np.stack(svs[1:], -1), g[f'{tag}_sv'])
    t_ref = dt.datetime(2018, 11, 12, 23, 0, 2)
    svs = orbits.get_sv(str(d / 'S1_sv_file.txt'), t_ref + dt.timedelta(seconds=40), 15)
    assert np.array_equal([(t - t_ref).total_seconds() for t in svs[0]], g['cut_t']) and np.array_equal(np.stack(svs[1:], -1), g['cut_sv'])
    svs = orbits.get_sv(str(d / 'S1_orbit_example.EOF'), t_ref, 3 * 60)          # non-standard EOF name must not be filtered out
    assert len(svs[0]) == 8
    times = orbits.read_txt_file(str(d / 'S1_sv_file.txt'))[0]
    assert np.array_equal(orbits.cut_times(times, t_ref, pad=5), g['cut_mask_5'])
    assert np.array_equal(orbits.cut_times(times, times[4], pad=15), g['cut_mask_15'])
    for bad in ('incorrect_file.txt', 'no_exist.txt'):                               # test_get_sv_3 / _4
        with pytest.raises(ValueError):
            orbits.get_sv(str(d / bad), t_ref, 3 * 60)
    orb = orbits.Orbit.from_file(str(d / 'S1_sv_file.txt'), t_ref, 600)
    assert orb.time.size == 8 and orb.direction() == 'desc' and np.all(np.diff(orb.time) == 10.0)
    with pytest.raises(RuntimeError):
        orbits.Orbit(list(times[:3]), np.zeros((3, 3)), np.zeros((3, 3)))


def test_oracle_orbit_geometry():
    """The oracle's zero-Doppler solve: (S - T) . V = 0 at the returned time, unit look vectors, Hermite reproduces the
    state vectors at the nodes."""
    import datetime as dt
    from oracle import raider_oracle as O
    from raider_amd import orbits
    d = REPO / 'tests' / 'golden' / 'orbit_files'
    orb = orbits.Orbit.from_file(str(d / 'S1_sv_file.txt'), dt.datetime(2018, 11, 12, 23, 0, 2), 600)
    p, v = O.orbit_hermite(orb.time, orb.position, orb.velocity, orb.time[2:6])
    np.testing.assert_allclose(p, orb.position[2:6], rtol=0, atol=1e-6); np.testing.assert_allclose(v, orb.velocity[2:6], rtol=0, atol=1e-9)
    # ground targets ~ 250-450 km to the right of the (descending) track
    mid, vmid = O.orbit_hermite(orb.time, orb.position, orb.velocity, [35.0])
    lon_s, lat_s, _ = O.ecef2lla(mid[:, 0], mid[:, 1], mid[:, 2])
    lat = lat_s[0] + np.linspace(-0.1, 0.1, 5)[:, None] + np.zeros((1, 6)); lon = lon_s[0] - np.linspace(2.5, 4.5, 6)[None, :] + np.zeros((5, 1))
    xyz = np.stack(O.lla2ecef(lat, lon, np.zeros_like(lat)), -1)
    los, az, rg = O.orbit_look_vectors(orb.time, orb.position, orb.velocity, xyz)
    assert np.isfinite(los).all()
    np.testing.assert_allclose(np.linalg.norm(los, axis=-1), 1.0, rtol=0, atol=1e-15)
    S, V = O.orbit_hermite(orb.time, orb.position, orb.velocity, az.ravel())
    dop = np.sum((S - xyz.reshape(-1, 3)) * V, -1) / (rg.ravel() * np.linalg.norm(V, axis=-1))
    assert np.abs(dop).max() < 1e-9                               # cos of the squint angle
    up = O.getZenithLookVecs(lat, lon, 0)
    inc = np.degrees(np.arccos(np.sum(los * up, -1)))
    assert inc.min() > 15 and inc.max() < 50


def test_cube_file_variables_are_read_lazily(tmp_path):
    """Processed-cube files: variables are read on first use (a ray-traced run never touches the *_total fields), values and
    attributes survive the NetCDF-3 round trip, and the cheap NaN test agrees with np.isnan(...).any()."""
    from scipy.io import netcdf_file
    from raider_amd.delay import _has_nan
    from raider_amd.delayFcns import _read_cube_file
    p = tmp_path / 'cube.nc'
    rng = np.random.default_rng(0)
    wet = rng.random((4, 5, 6)).astype(np.float32); tot = rng.random((4, 5, 6))
    with netcdf_file(str(p), 'w', version=2) as f:
        for d, n in (('z', 4), ('y', 5), ('x', 6)):
            f.createDimension(d, n)
            f.createVariable(d, 'f8', (d,))[:] = np.arange(n, dtype=np.float64)
        f.createVariable('wet', 'f4', ('z', 'y', 'x'))[:] = wet
        f.createVariable('wet_total', 'f8', ('z', 'y', 'x'))[:] = tot
        pj = f.createVariable('proj', 'i4', ())
        pj.data[()] = 0
        pj.crs_wkt = 'GEOGCRS["WGS 84",ID["EPSG",4326]]'
    v = _read_cube_file(str(p))
    assert callable(v['wet_total']._data) and callable(v['wet']._data)            # nothing read yet
    assert v['proj'].attrs['crs_wkt'].endswith('4326]]')
    got = v['wet'][:]
    assert got.dtype == np.float32 and np.array_equal(got, wet) and v['wet'].data.flags.owndata
    assert not callable(v['wet']._data) and callable(v['wet_total']._data)        # only what was asked for
    assert np.array_equal(np.asarray(v['wet_total']), tot)
    big = rng.random((70, 40, 40))
    assert not _has_nan(big) and not _has_nan(big[::2])
    big[33, 7, 9] = np.nan
    assert _has_nan(big) and _has_nan(big[1::2]) and _has_nan(big.astype(np.float32)) and not _has_nan(np.zeros(5))
    big[33, 7, 9] = np.inf
    assert not _has_nan(big)


class _SV:        # (module level: picklable)
    def __init__(self, time, position, velocity):
        self.time, self.position, self.velocity = time, position, velocity


class _Holder:
    pass


def test_get_sv_reads_an_isce2_style_shelve(tmp_path):
    """losreader.py:360-362,399-426: the last resort of get_sv is a shelve holding `frame.orbit.stateVectors`."""
    import datetime
    import shelve
    from raider_amd import orbits
    t0 = datetime.datetime(2020, 1, 30, 13, 52, 45)
    frame = _Holder(); frame.orbit = _Holder()
    frame.orbit.stateVectors = [_SV(t0 + datetime.timedelta(seconds=10 * i), [7.0e6 + i, 1.0 * i, -2.0 * i], [1.0, 7.5e3 + i, 0.5]) for i in range(-70, 71)]
    path = tmp_path / 'frame_shelve'
    with shelve.open(str(path), 'c') as db:
        db['frame'] = frame
    t, x, y, z, vx, vy, vz = orbits.get_sv(str(path), t0, 600)
    assert len(t) == 119 and t[0] == t0 - datetime.timedelta(seconds=590) and x[0] == 7.0e6 - 59 and vy[-1] == 7.5e3 + 59   # cut to |dt| < pad
    orb = orbits.Orbit(t, np.stack([x, y, z], -1), np.stack([vx, vy, vz], -1))
    assert orb.time.size == 119
    empty = _Holder(); empty.orbit = _Holder(); empty.orbit.stateVectors = []
    with shelve.open(str(tmp_path / 'empty_shelve'), 'c') as db:
        db['frame'] = empty
    with pytest.raises(ValueError, match='cannot parse'):
        orbits.get_sv(str(tmp_path / 'empty_shelve'), t0, 600)


def test_field_interpolators_carry_no_hand_over_state():
    """ADVICE r2 / VERDICT r3: the wet -> hydro hand-over of FieldInterpolator (a result cached under a digest of ALL of xi, hashed on
    both calls) is gone: the two objects are stateless views of one device cube, each call gathers its own field
    (tests/test_gpu_api.py::test_interpolator_calls_are_stateless does the in-place-edit check on the GPU)."""
    from raider_amd.delayFcns import FieldInterpolator

    class _Cube:
        grid = (np.arange(2.0), np.arange(2.0), np.arange(2.0))
        def __init__(self): self.calls = []
        def interp(self, pts, field=None):
            self.calls.append((pts.copy(), field))
            out = [None, None]; out[field] = pts[..., 0] * (field + 1)
            return tuple(out)
    c = _Cube()
    w, h = FieldInterpolator(c, 0), FieldInterpolator(c, 1)
    assert not any(k.startswith('_') for k in vars(w))              # no _cache / _sibling / digest
    p = np.array([[0.25, 0.5, 0.5], [0.75, 0.5, 0.5]])
    a = w(p)
    p[0, 0] = 0.5                                                   # edited in place between the two calls
    b = h(p)
    assert np.array_equal(a, [0.25, 0.75]) and np.array_equal(b, [1.0, 1.5]) and [f for _, f in c.calls] == [0, 1]


def test_envi_header_names_the_rasters_own_crs(tmp_path):
    """a UTM raster must not be declared geographic; a CRS without an ENVI spelling gets no map info at all."""
    from raider_amd.utilFcns import writeArrayToRaster
    try:
        import rasterio  # noqa: F401
        pytest.skip('rasterio writes the raster itself')
    except ImportError:
        pass
    a = np.arange(12, dtype=np.float64).reshape(3, 4)
    gt = (500000.0, 30.0, 0.0, 3700000.0, 0.0, -30.0)
    writeArrayToRaster(a, tmp_path / 'utm.envi', proj='EPSG:32611', gt=gt)
    hdr = (tmp_path / 'utm.hdr').read_text()
    assert 'map info = {UTM, 1, 1, 500000, 3700000, 30, 30, 11, North, WGS-84}' in hdr and 'Geographic' not in hdr
    writeArrayToRaster(a, tmp_path / 'ps.envi', proj='EPSG:3413', gt=gt)
    assert 'map info' not in (tmp_path / 'ps.hdr').read_text()
    writeArrayToRaster(a, tmp_path / 'll.envi', gt=(-118.0, 0.01, 0.0, 34.0, 0.0, -0.01))
    assert 'Geographic Lat/Lon' in (tmp_path / 'll.hdr').read_text()


def test_round4_host_logic_without_a_gpu(tmp_path, monkeypatch):
    """Host-side pieces of round 4 that need no device: the file-identity cache of opened model files (same file -> same object; a
    rewritten file is read again; RAIDER_HIP_FILE_CACHE=0 switches it off), the byte model that picks on-the-fly blending for a rank's
    station block, the pinned pool's per-rank limit, and the result list that carries the device's NaN verdict."""
    import os
    from scipy.io import netcdf_file
    from raider_amd import delayFcns as F
    from raider_amd import _pinned
    from raider_amd.delay import _Result
    from raider_amd.distributed import blend_on_the_fly_pays

    def write(path, v):
        with netcdf_file(str(path), 'w', version=2) as f:
            f.createDimension('z', 3); f.createVariable('z', 'f8', ('z',))[:] = [0.0, 1.0, v]
    p = tmp_path / 'm.nc'
    write(p, 2.0)
    F.clear_file_cache()
    a, get = F._load_fields(str(p)); b, _ = F._load_fields(p)
    assert a is b and np.array_equal(get('z'), [0.0, 1.0, 2.0])
    write(p, 5.0)
    os.utime(p, ns=(os.stat(p).st_atime_ns, os.stat(p).st_mtime_ns + 7_000_000))
    c_, get2 = F._load_fields(str(p))
    assert c_ is not a and np.array_equal(get2('z'), [0.0, 1.0, 5.0])
    monkeypatch.setenv('RAIDER_HIP_FILE_CACHE', '0')
    assert F._load_fields(str(p))[0] is not c_
    monkeypatch.delenv('RAIDER_HIP_FILE_CACHE')
    assert F._file_key(tmp_path / 'missing.nc') is None
    F.clear_file_cache()

    class _C:                                               # (what blend_on_the_fly_pays reads off a Cube)
        shape = (1000, 1000, 50); dtype = np.float32
    assert blend_on_the_fly_pays(_C, 625_000) and not blend_on_the_fly_pays(_C, 5_000_000)
    _C.dtype = np.float64
    assert blend_on_the_fly_pays(_C, 3_500_000)             # an f64 blend moves twice the bytes per cell

    monkeypatch.delenv('RAIDER_HIP_PINNED_POOL_BYTES', raising=False)
    monkeypatch.setenv('LOCAL_WORLD_SIZE', '8')
    assert _pinned._limit() == (4 << 30) // 8               # eight ranks of a node page-lock together what one process would
    monkeypatch.setenv('RAIDER_HIP_PINNED_POOL_BYTES', '123')
    assert _pinned._limit() == 123

    r = _Result([np.zeros(2), np.ones(2)])
    w, h = r
    assert isinstance(r, list) and r.has_nan is None and len(r) == 2 and h[0] == 1.0
    r.has_nan = True
    assert r.has_nan is True and _Result().has_nan is None  # (per instance, not shared)


def test_round6_host_logic_without_a_gpu():
    """Round 6, the parts that need no GPU: the real level axes shipped as data (models/model_levels.py: ERA5's 145 heights, HRRR's 50 + 7), a
    synthetic cube on a given z axis, the byte model that routes a two-epoch station query, and the scaling-efficiency arithmetic of an N > 1
    bench line."""
    import importlib.util
    from raider_amd.synthetic import synthetic_cube, real_level_heights
    from raider_amd import distributed as D
    e, h = real_level_heights('era5'), real_level_heights('hrrr')
    assert e.shape == (145,) and h.shape == (57,) and np.all(np.diff(e) > 0) and np.all(np.diff(h) > 0)
    assert e[0] == -500.0 and e[-1] == 80301.65 and h[0] == -500.0 and abs(h[-1] - 26158.0385) < 1e-9 and 0.0 in e and 0.0 in h
    c = synthetic_cube(6, 7, h.size, seed=0, zs=h)
    assert c['wet'].shape == (57, 6, 7) and c['wet'].dtype == np.float32 and np.array_equal(c['zs'], h)
    assert np.allclose(c['hydro_total'][-1], 0.0) and (np.diff(c['hydro_total'], axis=0) < 0).all()      # totals integrate downwards from the top
    with pytest.raises(ValueError):
        synthetic_cube(6, 7, 5, zs=h)                          # nz must match
    with pytest.raises(ValueError):
        synthetic_cube(6, 7, 57, zs=h[::-1])                   # ascending
    assert np.array_equal(synthetic_cube(5, 5, 8, seed=3)['zs'], np.round(-100 + 41000.0 * np.linspace(0, 1, 8) ** 2, 3))      # the default axis is unchanged

    class Shape:
        def __init__(self, shape, dtype): self.shape, self.dtype = shape, dtype
    hrrr = Shape((1000, 1000, 50), np.float32)
    assert D.blend_on_the_fly_pays(hrrr, 625_000) and D.blend_on_the_fly_pays(hrrr, 1_800_000) and not D.blend_on_the_fly_pays(hrrr, 2_000_000)
    assert not D.blend_on_the_fly_pays(hrrr, 5_000_000)                                                   # one GPU holding all of configs[4]: the paired cube
    assert D.blend_on_the_fly_pays(Shape((1000, 1000, 50), np.float64), 3_500_000)                        # f64 cells cost twice as much to blend

    spec = importlib.util.spec_from_file_location('bench_for_test', Path(__file__).resolve().parent.parent / 'bench.py')
    bench = importlib.util.module_from_spec(spec); spec.loader.exec_module(bench)
    one, eff = bench.scaling_reference('strong', 40.0, 1.0e8, 8, 5.5, 3, 'x')
    assert abs(eff - 40.0 / (8 * 5.5)) < 1e-15 and abs(one['value'] - 1.0e8 / 0.040) < 1e-3 and one['steps'] == 3
    one, eff = bench.scaling_reference('weak', 6.0, 1.6e7, 8, 6.3, 3, 'x')
    assert abs(eff - 6.0 / 6.3) < 1e-15 and abs(one['value'] - 1.6e7 / 0.006) < 1e-3


def test_bench_dump_outputs_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    """bench.py --dump-outputs: arrays within the budget are written whole; above it every array keeps the SAME seeded sample of its
    elements (sorted flat indices), from run to run, and the files stay within the budget; non-float arrays are written as float64."""
    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location('bench_for_test', Path(__file__).resolve().parent.parent / 'bench.py')
    bench = importlib.util.module_from_spec(spec); spec.loader.exec_module(bench)
    w = torch.arange(300 * 200, dtype=torch.float64).reshape(300, 200); h = -w.float(); n = torch.arange(7, dtype=torch.int32)
    bench.dump_outputs(str(tmp_path / 'whole'), {'wet': w, 'hydro': h, 'n': n})
    assert np.array_equal(np.load(tmp_path / 'whole' / 'wet.npy'), w.reshape(-1).numpy()) and np.load(tmp_path / 'whole' / 'hydro.npy').dtype == np.float32
    assert np.load(tmp_path / 'whole' / 'n.npy').dtype == np.float64
    monkeypatch.setattr(bench, 'DUMP_BYTES_MAX', 200_000)
    for run in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / run), {'wet': w, 'hydro': h})
    a, b = np.load(tmp_path / 'a' / 'wet.npy'), np.load(tmp_path / 'b' / 'wet.npy')
    assert np.array_equal(a, b) and 0 < a.size < w.numel() and np.all(np.diff(a) > 0)          # wet = its own flat index: sorted, distinct
    assert np.array_equal(np.load(tmp_path / 'a' / 'hydro.npy'), -a.astype(np.float32))       # the same elements of every array
    assert sum(f.stat().st_size for f in (tmp_path / 'a').iterdir()) <= 200_000
