#!/usr/bin/env python3
"""tests/golden/g23_seasonal.npz: the reference's own seasonal fits - `RaiderStats(csv, 'ZTD', grid_seasonal_phase=True,
grid_seasonal_absolute_phase=True, period_limit=...)` (cli/statsPlot.py), whose constructor runs `create_DF` WHOLE on a CSV this tool
writes: the pandas reader, the gridding, one `scipy.optimize.curve_fit` per station in a process pool (`_amplitude_and_phase`,
:2311-2479) and the groupby passes behind the fourteen grid_seasonal_* maps (:1796-2309).

    python tools/gen_golden_seasonal.py [--out ...] [--seed N]        (no GPU; needs pandas, scipy, matplotlib and the reference)

The reference is imported as tools/gen_golden_grid_stats.py imports it (its containment stand-in for the R-tree included).

The scene: the 3 x 2 one-degree grid of g21 / g22 (lon -118 .. -115, lat 33 .. 35), 760 daily dates from 2019-03-01 (2.08 years), nine
stations, an annual line of amplitude 0.03 on 2.4 with noise 0.01, phases spread over the circle:
  cell (0, 0)   three fitted stations with 15, 25 and 35 % holes, and the station WITHOUT A ROW (absent from the CSV, an all-NaN column);
  cell (2, 1)   two fitted stations with 10 and 30 % holes;
  cell (1, 1)   one fitted station (25 % holes);
  cell (1, 0)   only unfitted stations: one lacks its first 400 dates (span < 2 years), one has 60 % holes (below min_frac);
  the other two cells are empty.
Cells with several fitted stations hold different row counts, so the absolute maps differ from the plain ones (asserted).

Recorded: ids, lon, lat [N]; t [D] POSIX seconds; values [D, N] as pandas parsed them; plotbbox, grid_dim, spacing;
  fixed_<col> [N]   the reference's seven station columns for period_limit = 1.0, and fixed_<map> [ny, nx] its fourteen maps;
  free_<col> [N]    the seven station columns for period_limit = 0.0 (the reference's default: a free period);
  ld_fixed_<col>, ld_free_<col> [N]   the columns of the extended-precision (np.longdouble) restatement tests/seasonal_model.py: the
                    closed form at one year; the dense scan plus golden-section refinement of R(w) over periods 0.5 .. 2 years;
  gap_fixed_<col>, gap_free_<col> [N]   |reference - restatement| per station;
  ref_reached_minimum [N]   free period: the reference's residual sum seasonalfit_rmse^2 (n - 2) is within 1e-6 relative of the restated
                    minimum.  The tool ASSERTS that at least four fitted stations carry the flag and that every fitted station's reference
                    period lies inside 0.5 .. 2 years.
The maxima of the gaps are printed (DESIGN 5k quotes them) and kept in _meta.
"""
import argparse
import json
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tools'))

from gen_golden_grid_stats import reference_module          # noqa: E402
from tests import seasonal_model as M                       # noqa: E402

W, S, ND = -118.0, 33.0, 760
#            ix iy holes  kind
STATIONS = ((0, 0, 0.15, 'fit'), (0, 0, 0.25, 'fit'), (0, 0, 0.35, 'fit'), (0, 0, 1.00, 'rowless'), (2, 1, 0.10, 'fit'), (2, 1, 0.30, 'fit'),
            (1, 1, 0.25, 'fit'), (1, 0, 0.25, 'short'), (1, 0, 0.60, 'sparse'))
MAPS = tuple(f'grid_seasonal_{a}{m}' for a in ('', 'absolute_') for m in ('phase', 'amplitude', 'period', 'phase_stdev', 'amplitude_stdev',
                                                                        'period_stdev', 'fit_rmse'))
BAND = (0.5, 2.0)
OVERSAMPLE = 8


def scene(seed):
    rng = np.random.default_rng(seed)
    n = len(STATIONS)
    lon = np.array([W + ix + rng.uniform(0.06, 0.94) for ix, _, _, _ in STATIONS])
    lat = np.array([S + iy + rng.uniform(0.06, 0.94) for _, iy, _, _ in STATIONS])
    dates = np.datetime64('2019-03-01') + np.arange(ND)
    t = dates.astype('datetime64[s]').astype(np.int64).astype(np.float64)
    phase = 2 * np.pi * (np.arange(n) + rng.uniform(0, 1, n)) / n
    v = 2.4 + 0.03 * np.sin(2 * np.pi * t[:, None] / M.YEAR + phase[None, :]) + 0.01 * rng.standard_normal((ND, n))
    for i, (_, _, holes, kind) in enumerate(STATIONS):
        gone = rng.uniform(size=ND) < holes
        if kind == 'fit':
            gone[0] = gone[-1] = False                      # the whole span
        if kind == 'short':
            gone[:400] = True
        if kind == 'rowless':
            gone[:] = True
        v[gone, i] = np.nan
    perm = rng.permutation(n)                               # stations do not come sorted by cell
    ids = np.array([f'S{i:03d}' for i in range(n)])
    return ids, lon[perm], lat[perm], dates, t, v[:, perm], [STATIONS[p][3] for p in perm]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(ROOT / 'tests' / 'golden' / 'g23_seasonal.npz'))
    ap.add_argument('--seed', type=int, default=24)
    a = ap.parse_args()
    ids, lon, lat, dates, t, v, kinds = scene(a.seed)
    n = lon.size
    import pandas as pd
    import scipy
    sp = reference_module()
    tmp = Path(tempfile.mkdtemp(prefix='g23_'))
    csv = tmp / 'stations.csv'
    with open(csv, 'w') as f:
        f.write('ID,Lat,Lon,Date,ZTD\n')
        for d in range(ND):
            for i in range(n):
                if not np.isnan(v[d, i]):
                    f.write(f'{ids[i]},{float(lat[i])!r},{float(lon[i])!r},{dates[d]},{float(v[d, i])!r}\n')
    out = dict(ids=ids, t=t, kinds=np.array(kinds))
    ref = {}
    for tag, limit in (('fixed', 1.0), ('free', 0.0)):
        o = sp.RaiderStats(str(csv), 'ZTD', workdir=str(tmp / tag), spacing=1, grid_seasonal_phase=True, grid_seasonal_absolute_phase=True,
                           period_limit=limit, numCPUs=2)
        if tag == 'fixed':                                  # the series as the reference parsed it (before its dropna of unfitted stations: rebuilt from the CSV's rows it kept)
            raw = pd.read_csv(csv, parse_dates=['Date'])
            vv = np.full((ND, n), np.nan); plo = lon.copy(); pla = lat.copy()
            day = raw['Date'].values.astype('datetime64[D]')
            for sid, lo_, la_, dd, z in zip(raw['ID'].values, raw['Lon'].values, raw['Lat'].values, day, raw['ZTD'].values):
                i = int(sid[1:]); vv[int((dd - dates[0]).astype(int)), i] = z; plo[i] = lo_; pla[i] = la_
            assert np.array_equal(np.isnan(vv), np.isnan(v))
            for sid, dd, z in zip(o.df['ID'].values, o.df['Date'].values.astype('datetime64[D]'), o.df['ZTD'].values):      # and the reference's frame agrees
                assert vv[int((dd - dates[0]).astype(int)), int(sid[1:])] == z
            out['values'], out['lon'], out['lat'] = vv, plo, pla
            out['plotbbox'] = np.array(o.plotbbox, dtype=np.float64); out['grid_dim'] = np.array(o.grid_dim, dtype=np.int64)
            out['spacing'] = np.float64(o.spacing)
            assert list(o.grid_dim) == [3, 2], o.grid_dim
            for name in MAPS:
                m = np.array(getattr(o, name), dtype=np.float64)
                assert m.shape == (2, 3), (name, m.shape)
                out[f'fixed_{name}'] = m
        cols = {}
        for c in M.REF_COLUMNS:
            d = getattr(o, c)
            cols[c] = np.array([d.get(s, np.nan) for s in ids], dtype=np.float64)
            out[f'{tag}_{c}'] = cols[c]
        ref[tag] = cols
    vv = out['values']
    fitted = ~np.isnan(ref['fixed']['ampfit'])
    assert [k == 'fit' for k in kinds] == fitted.tolist(), (kinds, fitted)
    assert np.array_equal(fitted, ~np.isnan(ref['free']['ampfit']))
    nobs = (~np.isnan(vv)).sum(axis=0)
    # the absolute maps differ from the plain ones where a cell holds several fitted stations
    multi = np.abs(out['fixed_grid_seasonal_absolute_amplitude'] - out['fixed_grid_seasonal_amplitude']) > 1e-9
    assert multi.sum() >= 2, 'two cells with several fitted stations of different row counts'
    assert np.isnan(out['fixed_grid_seasonal_amplitude']).sum() == 3, 'two empty cells and the cell of unfitted stations'

    # the extended-precision restatement
    ld = np.longdouble
    two_pi = 2.0 * np.pi
    w_fixed = np.array([(1 / 1.0) * (1 / M.YEAR) * two_pi])
    span = float(t.max() - t.min())
    delta = two_pi / (OVERSAMPLE * span)
    w_lo, w_hi = two_pi / (BAND[1] * M.YEAR), two_pi / (BAND[0] * M.YEAR)
    w_scan = w_lo + np.arange(int(np.floor((w_hi - w_lo) / delta)) + 1) * delta
    meta_gaps = {}
    for tag, omega, scan in (('fixed', w_fixed, False), ('free', w_scan, True)):
        res = M.restate(t, vv, omega, scan, 2.0, 0.6, dtype=ld)
        assert np.array_equal(res['fitted'] != 0, fitted), (tag, res['fitted'])
        cols = M.ref_columns(res, scan)
        for c in M.REF_COLUMNS:
            x = np.asarray(cols[c], dtype=np.float64)
            out[f'ld_{tag}_{c}'] = x
            out[f'gap_{tag}_{c}'] = np.abs(ref[tag][c] - x)
        out[f'ld_{tag}_rss'] = np.asarray(res['rss'], dtype=np.float64)
        if scan:
            out['ld_free_at_edge'] = np.asarray(res['at_edge'] != 0)
            ref_rss = ref['free']['seasonalfit_rmse'] ** 2 * (nobs - 2)
            reached = fitted & (np.abs(ref_rss - out['ld_free_rss']) <= 1e-6 * out['ld_free_rss'])
            out['ref_reached_minimum'] = reached
            out['free_ref_rss'] = ref_rss
            per = ref['free']['periodfit'][fitted]
            assert ((per >= BAND[0]) & (per <= BAND[1])).all(), f'a reference period outside the band: {per} (change the seed)'
            assert reached.sum() >= 4, f'the reference reached the minimum at {int(reached.sum())} fitted stations only (change the seed)'
            assert (ref_rss[fitted] >= out['ld_free_rss'][fitted] * (1 - 1e-9)).all(), 'the reference below the restated minimum'
            print(f'free period: the reference reached the least-squares minimum at {int(reached.sum())} of {int(fitted.sum())} fitted stations;'
                  f' residual ratio elsewhere up to {np.nanmax(ref_rss / out["ld_free_rss"]):.3f}')
            sel = reached
        else:
            sel = fitted
        for c in M.REF_COLUMNS:
            g = out[f'gap_{tag}_{c}'][sel]; x = np.abs(out[f'ld_{tag}_{c}'][sel])
            meta_gaps[f'{tag}_{c}'] = dict(max_abs=float(g.max()), max_rel=float((g / x).max()))
            print(f'{tag:5s} {c:17s} max |reference - restatement| = {g.max():.3e}  (relative {(g / x).max():.3e})')
    out['scan_omega'] = w_scan
    from oracle.refharness import ref_import
    out['_meta'] = np.array(json.dumps(dict(
        ref_import.provenance(), numpy=np.__version__, pandas=pd.__version__, scipy=scipy.__version__, seed=a.seed,
        route="RaiderStats(csv, 'ZTD', spacing=1, grid_seasonal_phase=True, grid_seasonal_absolute_phase=True, period_limit=1.0 | 0.0, numCPUs=2)",
        strtree='shapely.strtree.STRtree replaced by the containment query of tools/gen_golden_grid_stats.py',
        restatement='tests/seasonal_model.py in np.longdouble; free period: band 0.5 .. 2 years, oversample 8',
        gaps=meta_gaps, gaps_over='fixed: the fitted stations; free: the stations where the reference reached the minimum',
        generator='tools/gen_golden_seasonal.py, companion of oracle/refharness/gen_golden.py')))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(a.out, **out)
    print(a.out, Path(a.out).stat().st_size, 'bytes')


if __name__ == '__main__':
    main()
