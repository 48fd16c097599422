"""Seasonal fits of a clustered station network: raider_amd.seasonal_fits (one device call) for a fixed period and for a 0.5 .. 2-year scan,
each on host arrays and on device tensors, against the reference's route on the same machine's CPU threads: one
`scipy.optimize.curve_fit` per station with the reference's guess (FFT bin, std * sqrt 2, mean; phase 0), t in POSIX seconds and
maxfev = 1e6 (cli/statsPlot.py:2350-2367), restated here, in a pool of --threads processes as `create_DF` runs it (:1823).

Scene: the stations of tools/bench_grid_variogram.py (20 000, 70 % in 60 clusters, over 40 x 25 one-degree cells), D daily dates, an
annual line of amplitude 0.03 on 2.4 with noise 0.01 and phases over the circle, 25 % holes.

The CPU route is timed on --cpu-stations of the stations (every n-th one) and its time scaled to all of them - a full run takes minutes
per repeat; the record says so.  The pool's processes are started fresh (spawn) BEFORE the device is opened and never touch it.
Three ALTERNATED repeats (every route once per round) after one warm-up of each; median and span (max - min) per route; a route is
ahead only where the medians differ by more than both spans.  The record holds the scan's K and its count of at_edge stations.

    python tools/bench_seasonal.py [--stations 20000] [--dates 3650] [--cpu-stations 1600] [--threads 16] [--out profiles/r29_seasonal.json]
"""
import argparse
import json
import multiprocessing as mp
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
YEAR = 31556952.0


def reference_fit(args):
    """`_amplitude_and_phase` (:2346-2431) for one station -> (|A|, period in years, rmse), NaN where the reference passes NaN"""
    import warnings
    from scipy import optimize
    tt, yy, min_span, min_frac, period_limit = args
    nan = (np.nan, np.nan, np.nan)
    if tt.size < 2:
        return nan
    span = (tt.max() - tt.min()) / YEAR
    if not (span >= min_span and tt.size / (span * 365.25) >= min_frac):
        return nan
    ff = np.fft.fftfreq(len(tt), (tt[1] - tt[0]))
    Fyy = abs(np.fft.fft(yy))
    guess_freq = abs(ff[np.argmax(Fyy[1:]) + 1])
    guess = [np.std(yy) * 2.0 ** 0.5, 2.0 * np.pi * guess_freq, 0.0, np.mean(yy)]
    if period_limit != 0.0:
        w = (1 / period_limit) * (1 / YEAR) * (2.0 * np.pi)
        f = lambda t, A, p, c: A * np.sin(w * t + p) + c
        guess = [guess[0], 0.0, guess[3]]
    else:
        f = lambda t, A, w, p, c: A * np.sin(w * t + p) + c
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        try:
            popt, _ = optimize.curve_fit(f, tt, yy, p0=guess, maxfev=int(1e6))
        except (TypeError, RuntimeError):
            return nan
    if period_limit == 0.0:
        w = popt[1]
    r = yy - f(tt, *popt)
    return abs(popt[0]), 1 / ((w / (2.0 * np.pi)) * YEAR), (np.sum(r ** 2) / (r.size - 2)) ** 0.5


def make_values(lon, nd, seed=29):
    rng = np.random.default_rng(seed)
    n = lon.size
    t = (np.datetime64('2012-01-01') + np.arange(nd)).astype('datetime64[s]').astype(np.int64).astype(np.float64)
    ph = rng.uniform(-np.pi, np.pi, n)
    v = np.empty((nd, n))
    for d0 in range(0, nd, 256):                            # in slabs: the temporaries stay small
        sl = slice(d0, min(d0 + 256, nd))
        v[sl] = 2.4 + 0.03 * np.sin(2 * np.pi * t[sl, None] / YEAR + ph[None, :]) + 0.01 * rng.standard_normal((sl.stop - sl.start, n))
        v[sl][rng.random((sl.stop - sl.start, n)) < 0.25] = np.nan
    return t, v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--stations', type=int, default=20000)
    ap.add_argument('--dates', type=int, default=3650)
    ap.add_argument('--cpu-stations', type=int, default=1600)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default='profiles/r29_seasonal.json')
    a = ap.parse_args()
    from tools.bench_grid_variogram import make_scene
    lon, lat, _ = make_scene(a.stations, 1)
    t, v = make_values(lon, a.dates)
    pick = np.arange(0, a.stations, max(a.stations // a.cpu_stations, 1))[:a.cpu_stations]
    series = [(t[~np.isnan(v[:, i])], v[~np.isnan(v[:, i]), i]) for i in pick]
    pool = mp.get_context('spawn').Pool(a.threads)          # fresh processes, before the device is opened here; they never open it
    cpu = lambda limit: np.array(pool.map(reference_fit, [(tt, yy, 2.0, 0.6, limit) for tt, yy in series], chunksize=max(len(series) // (4 * a.threads), 1)))

    import scipy
    import torch
    import raider_amd as R
    from raider_amd import _lib as L
    ctx = R.Context.default()
    name, cus, _ = ctx.device_info()
    v_d = torch.from_numpy(v).cuda()

    def dev(**kw):
        r = R.seasonal_fits(t, v_d, ctx=ctx, **kw)
        torch.cuda.synchronize()
        return r
    scan_kw = dict(period_range=(0.5, 2.0))
    routes = {'fixed_host_arrays': lambda: R.seasonal_fits(t, v, period_limit=1.0, ctx=ctx), 'fixed_device_tensors': lambda: dev(period_limit=1.0),
              'fixed_cpu': lambda: cpu(1.0),
              'scan_host_arrays': lambda: R.seasonal_fits(t, v, ctx=ctx, **scan_kw), 'scan_device_tensors': lambda: dev(**scan_kw),
              'scan_cpu': lambda: cpu(0.0)}
    first = {k: f() for k, f in routes.items()}            # the warm-up of each, and the check
    check = {}
    for mode in ('fixed', 'scan'):
        got, want = first[f'{mode}_host_arrays'], first[f'{mode}_cpu']
        amp, per, rmse = np.asarray(got.amplitude)[pick], np.asarray(got.period)[pick], np.asarray(got.rmse)[pick]
        ok = ~np.isnan(amp) & ~np.isnan(want[:, 0])
        same = ok & (np.abs(rmse - want[:, 2]) <= 1e-6 * rmse)                     # the stations where the CPU route ended in the least-squares minimum
        big = lambda x: float(x[same].max()) if same.any() else None
        check[mode] = dict(fitted=int((~np.isnan(amp)).sum()), fitted_by_the_cpu_route=int((~np.isnan(want[:, 0])).sum()), cpu_route_reached_the_minimum=int(same.sum()),
                           cpu_rmse_below_device=int((ok & (want[:, 2] < rmse * (1 - 1e-9))).sum()),
                           largest_relative_amplitude_difference_where_it_did=big(np.abs(amp - want[:, 0]) / amp),
                           largest_relative_period_difference_where_it_did=big(np.abs(per - want[:, 1]) / per))
    times = {k: [] for k in routes}
    for _ in range(a.reps):
        for k, f in routes.items():
            t0 = time.perf_counter(); f(); times[k].append(time.perf_counter() - t0)
    pool.close(); pool.join()
    scale = a.stations / len(series)
    summary = {}
    for k, ts in times.items():
        s = dict(median=statistics.median(ts), span=max(ts) - min(ts), repeats=ts)
        if k.endswith('cpu'):
            s = dict(s, stations_timed=len(series), median_scaled_to_all_stations=s['median'] * scale, span_scaled_to_all_stations=s['span'] * scale)
        summary[k] = s
    for mode in ('fixed', 'scan'):
        c = summary[f'{mode}_cpu']
        for r in ('host_arrays', 'device_tensors'):
            s = summary[f'{mode}_{r}']
            s['ratio_cpu_scaled_over_this'] = c['median_scaled_to_all_stations'] / s['median']
            s['ahead_of_cpu_by_more_than_both_spans'] = bool(c['median_scaled_to_all_stations'] - s['median'] > c['span_scaled_to_all_stations'] + s['span'])
    sc = first['scan_host_arrays']
    row = dict(stations=a.stations, dates=a.dates, values=int((~np.isnan(v)).sum()), scan_frequencies=int(sc.omega_grid.size),
               scan_at_edge_stations=int(np.asarray(sc.at_edge).sum()), fitted_stations=int(np.asarray(sc.fitted).sum()),
               scan_golden_section_steps_median=float(np.nanmedian(np.asarray(sc.iterations))),
               cpu_route=f'scipy {scipy.__version__} curve_fit per station, the reference\'s guess and maxfev, spawn pool of {a.threads} processes, '
                         f'{len(series)} of {a.stations} stations timed and scaled',
               agreement=check, seconds=summary)
    print('# ' + ', '.join(f"{k} {s['median']:.4f} s (span {s['span']:.4f})" for k, s in summary.items()), file=sys.stderr, flush=True)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(dict(tool='bench_seasonal', device=name, compute_units=cus, source_hash=L.source_hash(), rows=[row]), indent=1) + '\n')
    print(json.dumps(row))


if __name__ == '__main__':
    main()
