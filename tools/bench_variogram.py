"""All-pair variograms of N random stations and D dates: time per call of raider_amd.pair_variogram on the GPU, against a chunked
NumPy all-pairs restatement on the same machine's CPUs and, for context, against the reference's 1000-pair sampling.

  device tensors, given edges     one pass over the pairs (rdr_pair_variogram)
  device tensors, default edges   two passes: the largest pair distance per date, then the bins (what station_variograms runs)
  host arrays, default edges      the same with upload of x, y, values and download of the sums
  numpy all pairs                 rows of the pair matrix in chunks over a thread pool (NumPy releases the GIL in its loops):
                                  np.sqrt(dx*dx + dy*dy), np.searchsorted(edges, h, 'left') - the count of edges below h, i.e. the
                                  bin rule of statsPlot.py:644 -, np.bincount with weights.  Capped at --numpy-cap seconds: where it
                                  does not finish, the pairs it got through and its pairs/s are reported and the full time is
                                  the extrapolation from that rate, marked as such.
  reference sampling              what `_get_samples` keeps: 1000 pairs per date, here drawn directly (the reference first lists
                                  and shuffles ALL pairs in Python, which is timed separately at N = 2000 only: at 20000 the list is
                                  2 x 10^8 tuples).  It is a different, cheaper computation - a sample, not the variogram of all pairs.

Every GPU figure: 2 warm-up calls, a window of calls sized to >= 0.2 s and ended by a device synchronise, --reps windows, their
median and span (max - min).

    python tools/bench_variogram.py [--sizes 2000,10000,20000] [--dates 1,8] [--reps 5] [--numpy-cap 10] [--threads 16]
                                    [--out profiles/r25_variogram.json]
Prints ONE JSON line."""
import argparse
import itertools
import json
import random
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def timed(fn, sync, reps):
    fn(); fn(); sync()
    t0 = time.perf_counter(); fn(); sync(); once = time.perf_counter() - t0
    inner = max(1, int(np.ceil(0.2 / max(once, 1e-5))))
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        sync()
        ms.append((time.perf_counter() - t0) * 1e3 / inner)
    return dict(ms=statistics.median(ms), span_ms=max(ms) - min(ms), calls_per_window=inner, windows_ms=ms)


def numpy_all_pairs(x, y, v, edges, cap_s, threads, rows_per_chunk=64):
    """-> (count, lag, gam, pairs done, seconds, finished)"""
    n, D, B = x.size, v.shape[0], edges.size - 1
    t_end = time.perf_counter() + cap_s

    def chunk(i0):
        if time.perf_counter() > t_end:
            return None
        i1 = min(i0 + rows_per_chunk, n - 1)
        cnt = np.zeros((D, B + 2), dtype=np.int64); lag = np.zeros((D, B + 2)); gam = np.zeros((D, B + 2))
        pairs = 0
        for i in range(i0, i1):
            dx = x[i] - x[i + 1:]; dy = y[i] - y[i + 1:]
            h = np.sqrt(dx * dx + dy * dy)
            k = np.searchsorted(edges, h, side='left')             # edges below h: bin k - 1, 0 and B + 1 are outside
            for d in range(D):
                g = 0.5 * np.square(v[d, i] - v[d, i + 1:])
                ok = ~np.isnan(g)
                kk = k[ok]
                cnt[d] += np.bincount(kk, minlength=B + 2)
                lag[d] += np.bincount(kk, weights=h[ok], minlength=B + 2)
                gam[d] += np.bincount(kk, weights=g[ok], minlength=B + 2)
            pairs += h.size
        return cnt, lag, gam, pairs

    t0 = time.perf_counter()
    cnt = np.zeros((D, B + 2), dtype=np.int64); lag = np.zeros((D, B + 2)); gam = np.zeros((D, B + 2)); pairs = 0; finished = True
    with ThreadPoolExecutor(threads) as pool:
        for r in pool.map(chunk, range(0, n - 1, rows_per_chunk)):
            if r is None:
                finished = False
                continue
            cnt += r[0]; lag += r[1]; gam += r[2]; pairs += r[3]
    return cnt[:, 1:B + 1], lag[:, 1:B + 1], gam[:, 1:B + 1], pairs, time.perf_counter() - t0, finished


def reference_sampling(x, y, v, nsamp=1000):
    """the arithmetic of _get_samples .. _binned_vario on 1000 pairs per date (drawn directly), seconds per call"""
    rng = np.random.default_rng(0)
    n = x.size
    t0 = time.perf_counter()
    for d in range(v.shape[0]):
        i = rng.integers(0, n, nsamp); j = rng.integers(0, n, nsamp)
        h = np.sqrt((x[i] - x[j]) * (x[i] - x[j]) + (y[i] - y[j]) * (y[i] - y[j]))
        g = 0.5 * np.square(v[d, i] - v[d, j])
        e = np.linspace(0, np.nanmax(h) * 0.67, 20)
        for b in range(19):
            m = np.logical_and(e[b] < h, h <= e[b + 1])
            if m.any():
                np.nanmean(h[m]); np.nanmean(g[m])
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='2000,10000,20000')
    ap.add_argument('--dates', default='1,8')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--numpy-cap', type=float, default=10.0)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--out', default='profiles/r25_variogram.json')
    a = ap.parse_args()
    import torch
    import raider_amd as R
    from raider_amd import _lib as L
    from raider_amd import variogram as V
    ctx = R.Context.default()
    name, cus, _ = ctx.device_info()
    sync = torch.cuda.synchronize
    rows = []
    for n in (int(s) for s in a.sizes.split(',')):
        for D in (int(s) for s in a.dates.split(',')):
            rng = np.random.default_rng(n + D)
            x = rng.uniform(2e5, 8e5, n); y = rng.uniform(3.2e6, 4.0e6, n)
            v = 2.4 + 0.05 * rng.standard_normal((D, n)); v[:, ::97] = np.nan
            pairs = n * (n - 1) // 2
            tx, ty, tv = (torch.from_numpy(q).cuda() for q in (x, y, v))
            pv = V.pair_variogram(x, y, v)
            edges = pv.edges[0].copy()                              # one row for every side of the comparison
            te = torch.from_numpy(edges).cuda()
            row = dict(n=n, dates=D, pairs=pairs, pair_dates=pairs * D, bins=19)
            row['device_given_edges'] = timed(lambda: V.pair_variogram(tx, ty, tv, edges=te), sync, a.reps)
            row['device_default_edges'] = timed(lambda: V.pair_variogram(tx, ty, tv), sync, a.reps)
            row['host_default_edges'] = timed(lambda: V.pair_variogram(x, y, v), lambda: None, a.reps)
            row['device_pair_dates_per_s'] = pairs * D / (row['device_given_edges']['ms'] * 1e-3)
            cnt, lag, gam, done, secs, finished = numpy_all_pairs(x, y, v, edges, a.numpy_cap, a.threads)
            npy = dict(threads=a.threads, finished=finished, pairs_done=done, seconds=secs, pair_dates_per_s=done * D / secs)
            if finished:
                one = V.pair_variogram(x, y, v, edges=edges)
                npy['counts_equal'] = bool(np.array_equal(one.count, cnt))
                npy['largest_relative_sum_difference'] = float(max(np.abs(one.lag_sum - lag).max() / lag.max(), np.abs(one.gamma_sum - gam).max() / gam.max()))
                npy['full_seconds'] = secs
            else:
                npy['full_seconds_extrapolated'] = pairs / (done / secs)
            row['numpy_all_pairs'] = npy
            row['speedup_over_numpy_all_pairs'] = npy.get('full_seconds', npy.get('full_seconds_extrapolated')) * 1e3 / row['device_given_edges']['ms']
            row['reference_sampling_1000_pairs_s'] = statistics.median(reference_sampling(x, y, v) for _ in range(5))
            if n <= 2000 and D == 1:
                t0 = time.perf_counter()
                lst = list(itertools.combinations(range(n), 2)); random.shuffle(lst)
                row['reference_pair_listing_and_shuffle_s'] = time.perf_counter() - t0
                del lst
            rows.append(row)
            print(f"# n={n} D={D}: device {row['device_given_edges']['ms']:.3f} ms (given edges), {row['device_default_edges']['ms']:.3f} ms (default), "
                  f"host {row['host_default_edges']['ms']:.3f} ms; numpy {'%.2f s' % secs if finished else 'cap, %.3g pairs/s' % (done / secs)}", file=sys.stderr, flush=True)
    res = dict(tool='bench_variogram', device=name, compute_units=cus, source_hash=L.source_hash(), tile=V.TILE, rows=rows)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + '\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
