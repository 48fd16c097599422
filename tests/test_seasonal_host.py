"""Host side of the seasonal fits (raider_amd/seasonal.py; no GPU): the yardstick tests/seasonal_model.py against golden g23
(tools/gen_golden_seasonal.py: the reference's own RaiderStats run and a long-double restatement), SeasonalFits.as_reference and its
labels, the eligibility rule, every argument check of seasonal_fits / grid_seasonal (all of them come before a device is needed: this
machine may have none), and the raster files of GridSeasonal.to_rasters.

Bounds of the float64 yardstick against the long-double columns of g23 (n <= 760 rows, eps = 2^-53):
  fixed period  the closed form of sequential sums: relative n * eps * c with c the cancellation of the centred sums, at most 1e4 for
                an offset of 2.4 on an amplitude of 0.03 -> 1e-9 relative; phsfit = 182.625 sin(p) with p = p_c - w t_ref, w t_ref about
                310 rad -> 1e-10 days absolute.
  free period   R(w) is flat to round-off at its minimum: R = R0 + kappa / 2 (dw / delta)^2 with kappa about 0.1 of the explained sum per
                squared grid step at oversample 8, and a round-off of c eps Syy in R, c of order 10, gives dw <= sqrt(2 c eps Syy / kappa)
                delta, about 16 sqrt(eps) delta here; allowed: 64 sqrt(eps) delta.  periodfit follows with dw / w, phsfit with
                182.625 t_ref dw; the rmse is second order in dw (1e-9); the amplitude and the three sigmas are first order in
                dw / w <= 6e-8 with factors of order 1 .. 10 (1e-6).
"""
import math
from pathlib import Path

import numpy as np
import pytest

import raider_amd as R
from raider_amd import seasonal as S
from raider_amd import variogram as V
from tests import seasonal_model as M

GOLDEN = Path(__file__).resolve().parent / 'golden' / 'g23_seasonal.npz'
DAY = 86400.0


@pytest.fixture(scope='module')
def g23():
    return dict(np.load(GOLDEN))


def test_frequency_grid_restates_the_issue():
    t = np.arange(760) * DAY + 1.5e9
    w, scan = S.frequency_grid(t, period_limit=1.0)
    assert not scan and w.tolist() == [(1 / 1.0) * (1 / 31556952) * (2.0 * np.pi)]                       # (:2336)
    w, scan = S.frequency_grid(t, period_range=(0.5, 2.0))
    delta = 2 * np.pi / (8 * 759 * DAY)
    assert scan and w[0] == 2 * np.pi / (2.0 * S.YEAR) and np.allclose(np.diff(w), delta, rtol=1e-12, atol=0)
    assert w[-1] <= 2 * np.pi / (0.5 * S.YEAR) < w[-1] + delta
    assert S.frequency_grid(t, period_range=(0.5, 2.0), oversample=16)[0].size in (2 * w.size - 1, 2 * w.size)
    assert S.frequency_grid(t[:1], period_range=(0.5, 2.0))[0].tolist() == [w[0]]                        # one date: no span, one frequency


def test_golden_scene_is_what_the_issue_asks(g23):
    kinds = g23['kinds'].tolist()
    assert sorted(kinds) == sorted(['fit'] * 6 + ['short', 'sparse', 'rowless'])
    fitted = ~np.isnan(g23['fixed_ampfit'])
    assert fitted.tolist() == [k == 'fit' for k in kinds] and np.isnan(g23['values'][:, kinds.index('rowless')]).all()
    assert g23['values'].shape == (760, 9) and g23['grid_dim'].tolist() == [3, 2] and g23['plotbbox'].tolist() == [-118.0, -115.0, 33.0, 35.0]
    reached = g23['ref_reached_minimum']
    assert reached.sum() >= 4 and not reached[~fitted].any()
    per = g23['free_periodfit'][fitted]
    assert ((per >= 0.5) & (per <= 2.0)).all()
    # the derivable floor of the fixed-period phsfit gap: the reference's p += 3.14159 (:2416)
    assert np.nanmax(g23['gap_fixed_phsfit']) <= 182.625 * abs(3.14159 - np.pi) * 1.001
    # the absolute maps differ from the plain ones in the two cells with several fitted stations, and three cells are NaN in every map
    assert (np.abs(g23['fixed_grid_seasonal_absolute_amplitude'] - g23['fixed_grid_seasonal_amplitude']) > 1e-9).sum() == 2
    for m in S.MAPS:
        assert np.isnan(g23[f'fixed_{m}']).sum() == 3, m


def test_yardstick_fixed_period_against_long_double(g23):
    res = M.restate(g23['t'], g23['values'], S.frequency_grid(g23['t'], period_limit=1.0)[0], False, 2.0, 0.6)
    cols = M.ref_columns(res, False)
    fitted = res['fitted'] != 0
    assert fitted.tolist() == (~np.isnan(g23['ld_fixed_ampfit'])).tolist()
    for c in M.REF_COLUMNS:
        ld = g23[f'ld_fixed_{c}']
        assert np.isnan(cols[c][~fitted]).all(), c
        gap = np.abs(cols[c] - ld)[fitted]
        bound = 1e-10 if c == 'phsfit' else 1e-9 * np.abs(ld[fitted])
        print(c, gap.max())
        assert (gap <= bound).all(), (c, gap)
    assert np.isnan(res['sigma_omega']).all() and (res['at_edge'] == 0).all() and (res['iterations'][fitted] == 0).all()


def test_yardstick_free_period_against_long_double(g23):
    t = g23['t']
    omega, scan = S.frequency_grid(t, period_range=(0.5, 2.0))
    assert scan and np.array_equal(omega, g23['scan_omega'])
    res = M.restate(t, g23['values'], omega, True, 2.0, 0.6)
    cols = M.ref_columns(res, True)
    fitted = res['fitted'] != 0
    assert fitted.tolist() == (~np.isnan(g23['ld_free_ampfit'])).tolist()
    assert np.array_equal(res['at_edge'] != 0, g23['ld_free_at_edge']) and not (res['at_edge'] != 0).any()
    dw = 64 * math.sqrt(2.0 ** -53) * (omega[1] - omega[0])
    t_ref = 0.5 * (t.min() + t.max())
    rel = dict(periodfit=dw / omega[0], seasonalfit_rmse=1e-9, ampfit=1e-6, phsfit_c=1e-6, ampfit_c=1e-6, periodfit_c=1e-6)
    for c in M.REF_COLUMNS:
        ld = g23[f'ld_free_{c}']
        gap = np.abs(cols[c] - ld)[fitted]
        bound = 182.625 * t_ref * dw if c == 'phsfit' else rel[c] * np.abs(ld[fitted])
        print(c, gap.max(), np.max(bound))
        assert (gap <= bound).all(), (c, gap, bound)
    # the least-squares minimum is never above the reference's residual sum (its period lies inside the band at every station)
    assert (res['rss'][fitted] <= g23['free_ref_rss'][fitted] * (1 + 1e-9)).all()


def _fits(scan):
    n = 3
    a = lambda k: np.arange(n, dtype=np.float64) + k
    return R.SeasonalFits(nobs=np.array([5, 6, 7]), span_years=a(2), fitted=np.ones(n, bool), at_edge=np.zeros(n, bool), amplitude=a(10),
                          phase=np.array([0.0, np.pi / 2, -np.pi / 6]), offset=a(20), omega=a(30), period=a(40), frequency=1 / a(40), rss=a(50),
                          rmse=a(60), sigma_amplitude=a(70), sigma_phase=a(80), sigma_offset=a(90), sigma_omega=a(100), sigma_frequency=a(110),
                          scan=scan)


def test_as_reference_carries_the_reference_labels():
    for scan in (True, False):
        f = _fits(scan)
        r = f.as_reference()
        assert sorted(r) == sorted(M.REF_COLUMNS)
        assert np.allclose(r['phsfit'], [0.0, 182.625, -91.3125], rtol=0, atol=1e-12)                    # (365.25 / 2) sin(p)
        assert r['ampfit'] is f.amplitude and r['periodfit'] is f.period and r['seasonalfit_rmse'] is f.rmse and r['ampfit_c'] is f.sigma_amplitude
        if scan:                                             # (A, w, p, c): pcov[1, 1] is w's, pcov[2, 2] is p's
            assert r['periodfit_c'] is f.sigma_omega and r['phsfit_c'] is f.sigma_phase
        else:                                                # (A, p, c): THE QUIRK - "periodfit_c" is the phase's sigma, "phsfit_c" the offset's
            assert r['periodfit_c'] is f.sigma_phase and r['phsfit_c'] is f.sigma_offset


def test_eligibility_edges_of_the_yardstick():
    w = S.frequency_grid(np.zeros(1), period_limit=0.2)[0]
    days = np.arange(0.0, 101.0)
    t = 1.6e9 + days * DAY
    line = lambda tt: 2.0 + 0.5 * np.sin(w[0] * tt + 0.3) + 0.01 * np.cos(17.0 * tt / DAY)
    v = np.full((101, 8), np.nan)
    v[:, 0] = line(t)                                         # the whole axis
    v[::25, 1] = line(t[::25])                                # 5 rows = P + 2
    v[[0, 30, 60, 100], 2] = line(t[[0, 30, 60, 100]])        # 4 rows = P + 1: fitted
    v[[0, 50, 100], 3] = line(t[[0, 50, 100]])                # 3 rows = P: not fitted (the reference would, with an infinite covariance)
    v[40, 4] = 1.0                                            # one row
    v[:51, 6] = line(t[:51])                                  # span of exactly 50 days
    v[:50, 7] = line(t[:50])                                  # one day short of it
    span50 = 50 * DAY / M.YEAR
    res = M.restate(t, v, w, False, span50, 0.01)
    assert (res['fitted'] != 0).tolist() == [True, True, True, False, False, False, True, False]
    assert res['nobs'].tolist() == [101, 5, 4, 3, 1, 0, 51, 50] and res['span_years'][6] == span50 and res['span_years'][4] == 0
    assert np.isnan(res['span_years'][5]) and np.isnan(res['amplitude'][[3, 4, 5, 7]]).all()
    assert abs(res['amplitude'][0] - 0.5) < 0.01
    # a free period has four parameters: 4 rows are not enough, 5 are
    ws = S.frequency_grid(t, period_range=(0.1, 0.4))[0]
    res = M.restate(t, v, ws, True, span50, 0.01)
    assert (res['fitted'] != 0).tolist() == [True, True, False, False, False, False, True, False]
    assert abs(res['omega'][0] / w[0] - 1) < 1e-3 and (res['at_edge'][[0, 6]] == 0).all()      # (five rows 25 days apart alias: anything goes there)
    # min_frac counts the rows per day of the station's own span
    res = M.restate(t, v, w, False, 0.0, 0.5)
    assert (res['fitted'] != 0).tolist() == [True, False, False, False, False, False, True, True]


def test_arguments_are_checked_before_a_device_is_needed():
    when = np.datetime64('2020-01-01') + np.arange(50)
    v = np.zeros((50, 3))
    lon, lat = np.array([-117.5, -116.5, -115.5]), np.array([33.5, 34.5, 33.5])
    for call in (lambda **kw: R.seasonal_fits(when, v, **kw), lambda **kw: R.grid_seasonal(lon, lat, when, v, **kw)):
        with pytest.raises(ValueError, match='exactly one of period_limit'):
            call(period_limit=1.0, period_range=(0.5, 2.0))
        with pytest.raises(ValueError, match='exactly one of period_limit'):
            call(period_limit=None)
        for bad in (0.0, -1.0, float('nan'), float('inf')):
            with pytest.raises(ValueError, match='period_limit must be'):
                call(period_limit=bad)
        for bad in ((2.0, 0.5), (1.0, 1.0), (0.0, 1.0), (0.5, float('inf')), (1.0,), 3.0):
            with pytest.raises(ValueError, match='period_range'):
                call(period_range=bad)
        with pytest.raises(ValueError, match='more than 4096'):
            call(period_range=(0.001, 2.0), oversample=64)
        with pytest.raises(ValueError, match='oversample'):
            call(period_range=(0.5, 2.0), oversample=0)
        with pytest.raises(ValueError, match='min_span'):
            call(min_span=-1.0)
        with pytest.raises(ValueError, match='min_frac'):
            call(min_frac=float('nan'))
    with pytest.raises(TypeError, match='unknown argument'):
        R.grid_seasonal(lon, lat, when, v, period=1.0)
    with pytest.raises(ValueError, match='agree in D'):
        R.seasonal_fits(when[:49], v)
    with pytest.raises(ValueError, match='agree in D'):
        R.seasonal_fits(when, np.zeros((50, 3, 2)))
    with pytest.raises(ValueError, match='agree in N'):
        R.grid_seasonal(lon[:2], lat[:2], when, v)
    with pytest.raises(ValueError, match='dates'):
        R.seasonal_fits(np.arange(5000.0), np.zeros((5000, 1)))
    with pytest.raises(ValueError, match='NaT'):
        R.seasonal_fits(np.array(['2020-01-01', 'NaT'], dtype='datetime64[D]'), np.zeros((2, 1)))
    with pytest.raises(ValueError, match='finite'):
        R.seasonal_fits(np.array([0.0, np.nan]), np.zeros((2, 1)))
    with pytest.raises(TypeError, match='datetime64 or POSIX'):
        R.seasonal_fits(np.array(['a', 'b']), np.zeros((2, 1)))
    torch = pytest.importorskip('torch')
    with pytest.raises(TypeError, match='all NumPy arrays or all GPU tensors'):
        R.grid_seasonal(torch.from_numpy(lon), lat, when, v)
    with pytest.raises(TypeError, match='must live on the GPU'):
        R.seasonal_fits(when, torch.zeros(50, 3, dtype=torch.float64))
    with pytest.raises(TypeError, match='when is the date axis'):
        R.seasonal_fits(torch.arange(50.0), v)


def test_posix_seconds_of_datetime64():
    d = np.array(['1970-01-02', '2019-03-01'], dtype='datetime64[D]')
    assert S.posix_seconds(d).tolist() == [86400.0, 1551398400.0]
    assert S.posix_seconds(d.astype('datetime64[ns]')).tolist() == [86400.0, 1551398400.0]
    assert S.posix_seconds([1.5, 2]).tolist() == [1.5, 2.0]


def test_to_rasters_units_and_formats(tmp_path):
    grid = V.station_grid(np.array([-117.5, -115.5]), np.array([33.5, 34.5]))
    maps = {k: np.arange(6, dtype=np.float64).reshape(2, 3) / 8 + i for i, k in enumerate(S.MAPS)}
    for m in maps.values():
        m[1, 1] = np.nan
    res = R.GridSeasonal(grid=grid, fits=None, cell_means=None, **maps)
    assert len(S.MAPS) == 14 and res.plotbbox == [-118.0, -115.0, 33.0, 35.0]
    out = res.to_rasters(tmp_path / 'work', 'ZTD', unit='cm', stationsongrids=[-117.5, 33.5])
    assert sorted(out) == sorted(S.MAPS)
    # the reference's fourteen call sites (:1873-2309); 'days' and 'years' are not among the units whose format save_gridfile replaces (:456)
    want = {'phase': ('days', '%.1i'), 'amplitude': ('cm', '%.3f'), 'period': ('years', '%.2f'), 'phase_stdev': ('days', '%.1i'),
            'amplitude_stdev': ('cm', '%.3f'), 'period_stdev': ('years', '%.2e'), 'fit_rmse': ('cm', '%.3f')}
    for name, path in out.items():
        assert Path(path) == tmp_path / 'work' / f'ZTD_{name}.tif'
        key = name.replace('grid_seasonal_absolute_', '').replace('grid_seasonal_', '')
        unit, fmt = want[key]
        if name == 'grid_seasonal_absolute_fit_rmse':
            fmt = '%.2e'
        assert S.MAP_FILES[name] == (None if unit == 'cm' else unit, fmt)
        got, pb, sp, cfmt, sog, tl = R.load_gridfile(path, 'day' if unit in ('days', 'years') else 'cm')
        from raider_amd import tifflite
        tags = tifflite.read(path)[1]['tags']
        assert tags['gridfile_type'] == name and tags['unit'] == unit and tags['colorbarfmt'] == fmt
        assert cfmt == fmt and pb == res.plotbbox and sp == 1.0 and sog == [-117.5, 33.5] and tl is False
        assert np.array_equal(got, maps[name].astype(np.float32).astype(np.float64), equal_nan=True)
