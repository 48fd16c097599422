"""Host side of the gridded station statistics (raider_amd/station_stats.py: station_table, read_station_csv, save_gridfile,
load_gridfile; tifflite.write's tags; no GPU).

station_table is the row handling of RaiderStats._reader / create_DF (cli/statsPlot.py:1389-1437): convert_SI, the sigZTD filter, dropna,
the closed date interval.  The raster files follow save_gridfile / load_gridfile (:436-541).  tests/golden/g22_grid_stats.npz
(tools/gen_golden_grid_stats.py) holds the plotbbox and grid_dim the reference's create_DF arrived at."""
from pathlib import Path

import numpy as np
import pytest

import raider_amd as R
from raider_amd import station_stats as S
from raider_amd import tifflite
from raider_amd import variogram as V

GOLDEN = Path(__file__).resolve().parent / 'golden' / 'g22_grid_stats.npz'
D = lambda s: np.datetime64(s, 'ns')


def table():
    ids = np.array(['B', 'A', 'B', 'A', 'C', 'C', 'A'])
    lon = np.array([1.0, 2.0, 1.0, 2.0, 3.0, 3.0, 2.0]); lat = np.array([5.0, 6.0, 5.0, 6.0, 7.0, 7.0, 6.0])
    when = np.array(['2020-01-02', '2020-01-01', '2020-01-01', '2020-01-03', '2020-01-01', '2020-01-03', '2020-01-02'], dtype='datetime64[ns]')
    val = np.array([2.5, 2.25, 2.125, np.nan, 2.75, 3.0, 2.0])
    sig = np.array([0.001, 0.002, 0.02, 0.001, np.nan, 0.004, 0.003])
    return ids, lon, lat, when, val, sig


def test_station_table_drops_rows_with_a_nan_and_sorts():
    ids, lon, lat, when, val, _ = table()
    uid, ulon, ulat, uwhen, v = R.station_table(ids, lon, lat, when, val)
    assert uid.tolist() == ['A', 'B', 'C'] and ulon.tolist() == [2.0, 1.0, 3.0] and ulat.tolist() == [6.0, 5.0, 7.0]
    assert uwhen.dtype == np.dtype('datetime64[ns]') and uwhen.tolist() == [D('2020-01-01').item(), D('2020-01-02').item(), D('2020-01-03').item()]
    want = np.array([[2.25, 2.125, 2.75], [2.0, 2.5, np.nan], [np.nan, np.nan, 3.0]])      # A's NaN row is gone
    assert v.dtype == np.float64 and np.array_equal(v, want, equal_nan=True)
    # a NaN coordinate or time stamp drops the row as well; a station that loses every row is not in the table
    lon2 = lon.copy(); lon2[[0, 2]] = np.nan
    when2 = when.copy(); when2[4] = np.datetime64('NaT')
    uid, ulon, ulat, uwhen, v = R.station_table(ids, lon2, lat, when2, val)
    assert uid.tolist() == ['A', 'C'] and np.array_equal(v, [[2.25, np.nan], [2.0, np.nan], [np.nan, 3.0]], equal_nan=True)


def test_station_table_sigma_and_timeinterval():
    ids, lon, lat, when, val, sig = table()
    uid, _, _, uwhen, v = R.station_table(ids, lon, lat, when, val, sigma=sig, obs_errlimit=0.003)
    # sigma 0.02 and 0.004 are above the limit, the NaN sigma is a NaN in the row, 0.003 is kept (<=)
    assert uid.tolist() == ['A', 'B'] and uwhen.tolist() == [D('2020-01-01').item(), D('2020-01-02').item()]
    assert np.array_equal(v, [[2.25, np.nan], [2.0, 2.5]], equal_nan=True)
    # the limit is in metres, like sigma: the same rows in millimetres
    uid2, _, _, _, v2 = R.station_table(ids, lon, lat, when, val, sigma=sig, obs_errlimit=0.003, unit='mm')
    assert uid2.tolist() == ['A', 'B'] and np.array_equal(v2, (np.array([[2.25, np.nan], [2.0, 2.5]]) * 1.0) / 0.001, equal_nan=True)
    # the closed interval of days, as a string or as two dates
    for ti in ('2020-01-02 2020-01-03', [np.datetime64('2020-01-02'), np.datetime64('2020-01-03')]):
        uid, _, _, uwhen, v = R.station_table(ids, lon, lat, when, val, timeinterval=ti)
        assert uid.tolist() == ['A', 'B', 'C'] and uwhen.tolist() == [D('2020-01-02').item(), D('2020-01-03').item()]
        assert np.array_equal(v, [[2.0, 2.5, np.nan], [np.nan, np.nan, 3.0]], equal_nan=True)
    # a time of day counts with its day
    w = when + np.timedelta64(13, 'h')
    uid, _, _, uwhen, v = R.station_table(ids, lon, lat, w, val, timeinterval='2020-01-03 2020-01-03')
    assert uid.tolist() == ['C'] and uwhen.tolist() == [(D('2020-01-03') + np.timedelta64(13, 'h')).item()] and v.tolist() == [[3.0]]


@pytest.mark.parametrize('unit,factor', [('mm', 0.001), ('cm', 0.01), ('m', 1.0), ('km', 1000.0)])
def test_station_table_units(unit, factor):
    ids, lon, lat, when, val, _ = table()
    v = R.station_table(ids, lon, lat, when, val, unit=unit)[4]
    m = R.station_table(ids, lon, lat, when, val)[4]
    assert np.array_equal(v, m * 1.0 / factor, equal_nan=True)                            # convert_SI: val * SI['m'] / SI[unit]


def test_station_table_refusals():
    ids, lon, lat, when, val, _ = table()
    with pytest.raises(ValueError, match='User-specified output unit furlong not recognized.'):
        R.station_table(ids, lon, lat, when, val, unit='furlong')
    moved = lon.copy(); moved[6] = 2.5
    with pytest.raises(ValueError, match='station A has more than one location'):
        R.station_table(ids, moved, lat, when, val)
    twice = when.copy(); twice[6] = twice[1]
    with pytest.raises(ValueError, match='station A has 2 rows at 2020-01-01'):
        R.station_table(ids, lon, lat, twice, val)
    with pytest.raises(ValueError, match='same length'):
        R.station_table(ids, lon[:-1], lat, when, val)


@pytest.mark.parametrize('tcol', ['Date', 'Datetime'])
def test_read_station_csv(tmp_path, tcol):
    ids, lon, lat, when, val, sig = table()
    stamp = (lambda t: str(t.astype('datetime64[D]'))) if tcol == 'Date' else (lambda t: str((t + np.timedelta64(90, 'm')).astype('datetime64[s]')).replace('T', ' '))
    path = tmp_path / 'stations.csv'
    with open(path, 'w') as f:
        f.write(f'ID,Lat,Lon,{tcol},ZTD,sigZTD\n')
        for i in range(ids.size):
            f.write(f'{ids[i]},{float(lat[i])!r},{float(lon[i])!r},{stamp(when[i])},{"" if np.isnan(val[i]) else repr(float(val[i]))},'
                    f'{"" if np.isnan(sig[i]) else repr(float(sig[i]))}\n')
    uid, ulon, ulat, uwhen, v = R.read_station_csv(path, 'ZTD')
    shift = np.timedelta64(0, 'm') if tcol == 'Date' else np.timedelta64(90, 'm')
    # with a sigZTD column the rows with an empty sigma go (a NaN in the row); no limit: every other row stays
    assert uid.tolist() == ['A', 'B', 'C'] and ulon.tolist() == [2.0, 1.0, 3.0] and ulat.tolist() == [6.0, 5.0, 7.0]
    assert uwhen.tolist() == [(D(d) + shift).item() for d in ('2020-01-01', '2020-01-02', '2020-01-03')]
    assert np.array_equal(v, [[2.25, 2.125, np.nan], [2.0, 2.5, np.nan], [np.nan, np.nan, 3.0]], equal_nan=True)
    want = R.station_table(ids, lon, lat, when + shift, val, sigma=sig, obs_errlimit=0.003, timeinterval='2020-01-01 2020-01-02', unit='cm')
    got = R.read_station_csv(path, 'ZTD', obs_errlimit=0.003, timeinterval='2020-01-01 2020-01-02', unit='cm')
    for a, b in zip(got, want):
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')
    with pytest.raises(Exception, match=f'User-specified key ZWD not found in input file {path}. Must specify valid key.'):
        R.read_station_csv(path, 'ZWD')
    # the other column of the file can be read as the value, too
    assert np.array_equal(R.read_station_csv(path, 'sigZTD', obs_errlimit=1.0)[4][0], [0.002, 0.02, np.nan], equal_nan=True)


def test_gridfile_round_trip(tmp_path):
    a = np.array([[1.5, np.nan, 3.25], [4.0, 5.0, -6.5]])
    bbox = [-118.0, -115.0, 33.0, 35.0]
    p = tmp_path / 'ZTD_grid_delay_mean.tif'
    meta = R.save_gridfile(a, 'grid_delay_mean', p, bbox, 1.0, 'm', stationsongrids=[-117.5, 33.5], time_lines=[-117, -116])
    assert meta == {'gridfile_type': 'grid_delay_mean', 'plotbbox': '-118.0 -115.0 33.0 35.0', 'spacing': '1.0', 'unit': 'm', 'colorbarfmt': '%.2f',
                    'stationsongrids': '-117.5 33.5', 'time_lines': '-117 -116'}
    raw, prof = tifflite.read(p)
    assert raw.dtype == np.float32 and np.array_equal(raw, a.astype(np.float32), equal_nan=True)
    assert prof['nodata'] != prof['nodata'] and prof['crs'] == 4326 and prof['transform'] == (-118.0, 1.0, 0.0, 35.0, 0.0, -1.0)     # (:471)
    assert {k: prof['tags'][k] for k in meta} == meta
    got, pb, sp, fmt, sog, tl = R.load_gridfile(p, 'cm')
    assert np.array_equal(got, a * 100.0, equal_nan=True) and pb == bbox and sp == 1.0 and fmt == '%.2f' and sog == [-117.5, 33.5] and tl == [-117.0, -116.0]
    # the heatmap: int16, nodata 0, NaN cells written as 0 and read back as NaN
    h = np.array([[np.nan, 2.0, 3.0], [1.0, 10.0, 5.0]])
    p2 = tmp_path / 'ZTD_grid_heatmap.tif'
    meta = R.save_gridfile(h, 'grid_heatmap', p2, bbox, 0.5, 'm', colorbarfmt='%1i', dtype='int16', noData=0)
    assert meta['stationsongrids'] == 'False' and meta['time_lines'] == 'False' and meta['colorbarfmt'] == '%1i' and meta['spacing'] == '0.5'
    raw, prof = tifflite.read(p2)
    assert raw.dtype == np.int16 and raw.tolist() == [[0, 2, 3], [1, 10, 5]] and prof['nodata'] == 0.0
    assert prof['transform'] == (-118.0, 0.5, 0.0, 35.0, 0.0, -0.5)
    got, pb, sp, fmt, sog, tl = R.load_gridfile(p2, 'm')
    assert np.array_equal(got, h, equal_nan=True) and sp == 0.5 and fmt == '%1i' and sog is False and tl is False
    # a time unit as output: '%1i', and a 0 stays a 0
    assert R.save_gridfile(h, 'grid_heatmap', p2, bbox, 0.5, 'day', dtype='int16', noData=0)['colorbarfmt'] == '%1i'
    assert R.load_gridfile(p2, 'day')[0].tolist() == [[0, 2, 3], [1, 10, 5]]
    with pytest.raises(ValueError, match='fname is not a valid file'):
        bad = tmp_path / 'not_a.tif'
        bad.write_bytes(b'nothing of a TIFF')
        R.load_gridfile(bad, 'm')


def test_to_rasters_writes_the_maps_that_were_computed(tmp_path):
    grid = V.station_grid(np.array([-117.5, -115.5]), np.array([33.5, 34.5]))
    maps = {k: np.arange(6, dtype=np.float64).reshape(2, 3) + i for i, k in enumerate(S.MAPS)}
    maps['grid_heatmap'][0, 0] = np.nan
    res = R.GridStatistics(grid=grid, medians=False, **maps)
    out = res.to_rasters(tmp_path / 'work', 'ZTD', unit='m')
    assert sorted(out) == sorted(set(S.MAPS) - {'grid_delay_median', 'grid_delay_absolute_median'})
    for name, path in out.items():
        assert Path(path) == tmp_path / 'work' / f'ZTD_{name}.tif'
        raw, prof = tifflite.read(path)
        assert prof['tags']['gridfile_type'] == name and prof['tags']['plotbbox'] == '-118.0 -115.0 33.0 35.0'
        assert raw.dtype == (np.int16 if name == 'grid_heatmap' else np.float32)
        assert prof['tags']['colorbarfmt'] == ('%1i' if name == 'grid_heatmap' else '%.2f')
    assert tifflite.read(out['grid_heatmap'])[0][0, 0] == 0


def test_tifflite_tags_none_keeps_the_bytes(tmp_path):
    a = np.linspace(0.0, 1.0, 12, dtype=np.float32).reshape(3, 4)
    kw = dict(transform=(-118.0, 1.0, 0.0, 35.0, 0.0, -1.0), crs=4326, nodata=np.nan)
    tifflite.write(tmp_path / 'a.tif', a, **kw)
    tifflite.write(tmp_path / 'b.tif', a, tags=None, **kw)
    tifflite.write(tmp_path / 'c.tif', a, tags={}, **kw)
    tifflite.write(tmp_path / 'd.tif', a, tags={'unit': 'm', 'note': 'a < b & c'}, **kw)
    ref = (tmp_path / 'a.tif').read_bytes()
    assert (tmp_path / 'b.tif').read_bytes() == ref and (tmp_path / 'c.tif').read_bytes() == ref
    assert (tmp_path / 'd.tif').read_bytes() != ref
    raw, prof = tifflite.read(tmp_path / 'd.tif')
    assert np.array_equal(raw, a) and prof['tags']['unit'] == 'm' and prof['tags']['note'] == 'a < b & c'
    assert tifflite.read(tmp_path / 'a.tif')[1]['tags'] == {'AREA_OR_POINT': 'Area'}


@pytest.mark.parametrize('tag,spacing', [('s1', 1.0), ('s05', 0.5)])
def test_golden_g22_grid_is_station_grid_s(tag, spacing):
    g = np.load(GOLDEN)
    sg = V.station_grid(g['lon'], g['lat'], spacing=spacing)
    assert np.array(sg.extent, dtype=np.float64).tobytes() == g[f'{tag}_plotbbox'].tobytes()
    assert list(sg.grid_dim) == g[f'{tag}_grid_dim'].tolist() and sg.spacing == float(g[f'{tag}_spacing'])
    # the recorded heatmap is the count of stations with a row in station_grid's cells
    has_row = ~np.isnan(g['values']).all(axis=0)
    cnt = np.bincount(sg.cell[has_row], minlength=sg.gridpoints.shape[0]).astype(np.float64)
    heat = np.where(cnt > 0, cnt, np.nan).reshape(sg.grid_dim).T
    assert np.array_equal(heat, g[f'{tag}_grid_heatmap'], equal_nan=True)
    assert g[f'{tag}_grid_heatmap'].shape == (sg.grid_dim[1], sg.grid_dim[0])
