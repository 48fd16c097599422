"""Exponential variogram models of a clustered station network: raider_amd.fit_variograms (one device call per batch, each fit the exact
bounded minimum of the reference's objective) on device tensors and on host arrays, against the reference's route on the same machine's
CPU: one `scipy.optimize.least_squares` per row as raider_amd.fit_variogram runs it (`_fit_vario`, cli/statsPlot.py:661-701), in a pool
of --threads processes.

Scene: that of tools/bench_grid_variogram.py (20 000 clustered stations over 40 x 25 one-degree cells, 19 bins, plane removed, density
threshold 10).  grid_variograms(fit=False) gives the binned sums; the batches are the rows lag_sum / count that fitter='device' sends:
  total     one row per cell, of the --dates-total scene (the cells without a good date are all-NaN rows, status 1)
  per_date  one row per (cell, date), for each D of --dates

The CPU route is timed on --cpu-rows of the fitted rows of a batch (every n-th one) and its time scaled to all fitted rows - a full run
takes minutes; the record says so.  The pool's processes are started fresh (spawn) BEFORE the device is opened and never touch it.  Three
ALTERNATED repeats (every route once per round) after one warm-up of each; median and span (max - min) per route; a route is ahead only
where the medians differ by more than both spans.  On the rows the CPU route fitted, the record holds the share where scipy's cost
exceeds the device's by more than 1e-9 relative, the share where it is lower by more than that, and the median ratio.

    python tools/bench_variogram_fit.py [--dates 64 365] [--dates-total 64] [--cpu-rows 640] [--threads 16] [--out profiles/r30_variogram_fit.json]
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


def scipy_cost(args):
    """fit_variogram on one row -> scipy's cost at its solution (NaN where it raises)"""
    import warnings
    from raider_amd.variogram import fit_variogram
    h, g = args
    keep = ~(np.isnan(h) | np.isnan(g))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        try:
            return float(fit_variogram(h[keep], g[keep]).result.cost)
        except ValueError:
            return float('nan')


def rows_of(total, count, keep):
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where((count > 0) & keep, total / count, np.nan)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--stations', type=int, default=20000)
    ap.add_argument('--dates', type=int, nargs='+', default=[64, 365])
    ap.add_argument('--dates-total', type=int, default=64)
    ap.add_argument('--cpu-rows', type=int, default=640)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default='profiles/r30_variogram_fit.json')
    a = ap.parse_args()
    from tools.bench_grid_variogram import make_scene
    pool = mp.get_context('spawn').Pool(a.threads)          # fresh processes, before the device is opened here; they never open it

    import scipy
    import torch
    import raider_amd as R
    from raider_amd import _lib as L
    from raider_amd import variogram as V
    ctx = R.Context.default()
    name, cus, _ = ctx.device_info()

    batches = {}
    for nd in sorted(set(a.dates) | {a.dates_total}):
        lon, lat, v = make_scene(a.stations, nd)
        gv = V.grid_variograms(lon, lat, v, fit=False, ctx=ctx)
        good = gv.status != 1
        if nd in a.dates:
            k = good[:, :, None]
            batches[f'per_date_{nd}'] = (rows_of(gv.lag_sum, gv.count, k).reshape(-1, 19), rows_of(gv.gamma_sum, gv.count, k).reshape(-1, 19))
        if nd == a.dates_total:
            k = good.any(axis=1)[:, None]
            batches['total'] = (rows_of(gv.total_lag, gv.total_count, k), rows_of(gv.total_gamma, gv.total_count, k))
        del gv

    rows = []
    for tag, (h, g) in batches.items():
        h = np.ascontiguousarray(h); g = np.ascontiguousarray(g)
        h_d, g_d = torch.from_numpy(h).cuda(), torch.from_numpy(g).cuda()

        def dev():
            r = R.fit_variograms(h_d, g_d, ctx=ctx)
            torch.cuda.synchronize()
            return r
        first = R.fit_variograms(h, g, ctx=ctx)
        fitted = np.flatnonzero(first.status == 0)
        pick = fitted[::max(fitted.size // a.cpu_rows, 1)][:a.cpu_rows]
        sample = [(h[i], g[i]) for i in pick]
        cpu = lambda: np.array(pool.map(scipy_cost, sample, chunksize=max(len(sample) // (4 * a.threads), 1)))
        routes = {'device_tensors': dev, 'host_arrays': lambda: R.fit_variograms(h, g, ctx=ctx), 'cpu': cpu}
        warm = {k: f() for k, f in routes.items()}          # the warm-up of each, and the check
        assert [np.asarray(x.cpu()).tobytes() for x in warm['device_tensors']] == [x.tobytes() for x in first], 'device tensors and host arrays differ'
        c_cpu, c_dev = warm['cpu'], first.cost[pick]
        ok = ~np.isnan(c_cpu)
        ratio = c_cpu[ok] / c_dev[ok]
        times = {k: [] for k in routes}
        for _ in range(a.reps):
            for k, f in routes.items():
                t0 = time.perf_counter(); f(); times[k].append(time.perf_counter() - t0)
        scale = fitted.size / len(sample)
        summary = {k: dict(median=statistics.median(ts), span=max(ts) - min(ts), repeats=ts) for k, ts in times.items()}
        c = summary['cpu']
        c.update(rows_timed=len(sample), median_scaled_to_all_fitted_rows=c['median'] * scale, span_scaled_to_all_fitted_rows=c['span'] * scale)
        for k in ('device_tensors', 'host_arrays'):
            s = summary[k]
            s['ratio_cpu_scaled_over_this'] = c['median_scaled_to_all_fitted_rows'] / s['median']
            s['ahead_of_cpu_by_more_than_both_spans'] = bool(c['median_scaled_to_all_fitted_rows'] - s['median'] > c['span_scaled_to_all_fitted_rows'] + s['span'])
            s['behind_cpu_by_more_than_both_spans'] = bool(s['median'] - c['median_scaled_to_all_fitted_rows'] > c['span_scaled_to_all_fitted_rows'] + s['span'])
        flags = first.flags[fitted]
        row = dict(batch=tag, rows=int(h.shape[0]), columns=int(h.shape[1]), fitted_rows=int(fitted.size), status_counts={str(s): int((first.status == s).sum()) for s in range(4)},
                   range_at_floor=int((flags & V.AT_FLOOR != 0).sum()), range_at_ub=int((flags & V.AT_UB_A != 0).sum()), sill_at_zero=int((flags & V.SILL_ZERO != 0).sum()),
                   sill_at_ub=int((flags & V.SILL_UB != 0).sum()),
                   cpu_route=f'scipy {scipy.__version__} least_squares per row through fit_variogram, spawn pool of {a.threads} processes, {len(sample)} of '
                             f'{fitted.size} fitted rows timed and scaled',
                   cost=dict(rows_compared=int(ok.sum()), share_scipy_above_device_by_1e_9=float((ratio > 1 + 1e-9).mean()),
                             share_scipy_below_device_by_1e_9=float((ratio < 1 - 1e-9).mean()), median_ratio_scipy_over_device=float(np.median(ratio)),
                             largest_ratio=float(ratio.max()), smallest_ratio=float(ratio.min())),
                   seconds=summary)
        print(f'# {tag}: ' + ', '.join(f"{k} {s['median']:.4f} s (span {s['span']:.4f})" for k, s in summary.items())
              + f", cpu scaled {c['median_scaled_to_all_fitted_rows']:.2f} s", file=sys.stderr, flush=True)
        rows.append(row)
        del h_d, g_d
    pool.close(); pool.join()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(dict(tool='bench_variogram_fit', device=name, compute_units=cus, source_hash=L.source_hash(), stations=a.stations, rows=rows), indent=1) + '\n')
    print(json.dumps(rows))


if __name__ == '__main__':
    main()
