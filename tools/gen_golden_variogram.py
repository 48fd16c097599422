#!/usr/bin/env python3
"""tests/golden/g20_variogram.npz: the reference's own variogram chain (cli/statsPlot.py VariogramAnalysis: _get_samples, _get_XY,
_get_distances, _get_variogram, _binned_vario, _fit_vario) recorded on inputs small enough that it keeps EVERY pair.

Needs the reference tree and oracle/_ref (built by __graft_entry__.build()); no GPU.  The reference is imported in place through
oracle/refharness/ref_import.import_reference().  RAiDER.cli.statsPlot also imports shapely.strtree, which the harness stubs do not
have: an empty placeholder module of that name (with an STRtree attribute) is registered before the import - nothing of it is called.

Scenes:
  * 40 points, x / y in metres on an integer lattice (distinct nodes), three value sets a, b, c.  40 points are 780 pairs, fewer
    than the 1000 at which _get_samples starts to cut: the reference uses all pairs and its shuffle only reorders them.  This tool
    asserts that, and that the binned result equals a plain NumPy all-pairs restatement to round-off.
  * 9 points, below the density threshold of 10: _get_samples gives the empty sample.

The file holds the inputs and, per value set s: s_values, s_hmax (the largest of the reference's pair distances), s_edges (its
default bins, :638), s_count (pairs per bin by the masks of :644 on the reference's distances), s_hexp / s_vexp (_binned_vario),
s_fit (res_robust.x of _fit_vario with Nparm=3) and s_fit_spread: the largest |change| of each fitted parameter over 32 runs of
_fit_vario whose binned input was perturbed by relative 1e-12 (uniform in +-1e-12 per element) - the yardstick of the test's fit
tolerance.

    python tools/gen_golden_variogram.py [--out tests/golden/g20_variogram.npz]
"""
import argparse
import random
import sys
import types
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def reference_analysis():
    from oracle.refharness import ref_import
    ref_import.import_reference()
    if 'shapely.strtree' not in sys.modules:
        try:
            import shapely.strtree  # noqa: F401
        except ImportError:
            m = types.ModuleType('shapely.strtree')
            m.STRtree = type('STRtree', (), {})
            sys.modules['shapely.strtree'] = m
    from RAiDER.cli.statsPlot import VariogramAnalysis
    return VariogramAnalysis(None, None, 'ZTD')


def make_inputs():
    rng = np.random.default_rng(20)
    nodes = rng.choice(400 * 300, size=40, replace=False)
    x = (nodes % 400).astype(np.float64) * 500.0 + 300000.0          # a 200 km x 150 km network on a 500 m lattice
    y = (nodes // 400).astype(np.float64) * 500.0 + 3700000.0
    r = np.hypot(x - x.mean(), y - y.mean())
    vals = {
        'a': 0.02 * rng.standard_normal(40),
        'b': 1e-7 * (x - x.mean()) - 2e-7 * (y - y.mean()) + 0.01 * rng.standard_normal(40),
        'c': 2.4 + 0.05 * np.sin(r / 30000.0) + 0.005 * rng.standard_normal(40),
    }
    return x, y, vals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(ROOT / 'tests' / 'golden' / 'g20_variogram.npz'))
    a = ap.parse_args()
    va = reference_analysis()
    x, y, vals = make_inputs()
    out = dict(x=x, y=y)
    iu = np.triu_indices(40, 1)
    h_all = np.sqrt((x[iu[0]] - x[iu[1]]) * (x[iu[0]] - x[iu[1]]) + (y[iu[0]] - y[iu[1]]) * (y[iu[0]] - y[iu[1]]))
    for s, data in vals.items():
        random.seed(20)
        samples, indpars = va._get_samples(data)
        assert len(indpars) == 780 and len(set(indpars)) == 780, 'the reference did not keep all pairs'
        xx, yy = va._get_XY(x, y, indpars)
        dists = va._get_distances(np.array([[xx[:, 0], yy[:, 0]], [xx[:, 1], yy[:, 1]]]).T)
        vario = va._get_variogram(samples[:, 0], samples[:, 1])
        hexp, vexp = va._binned_vario(dists, vario)
        res, _, _ = va._fit_vario(hexp, vexp, model=va.__exponential__, x0=None, Nparm=3)
        edges = np.linspace(0, np.nanmax(dists) * 0.67, 20)
        count = np.array([np.logical_and(edges[b] < dists, dists <= edges[b + 1]).sum() for b in range(19)], dtype=np.int64)
        # the plain all-pairs restatement gives the same bins
        g_all = 0.5 * np.square(data[iu[0]] - data[iu[1]])
        assert np.sort(dists).tolist() == np.sort(h_all).tolist() or np.allclose(np.sort(dists), np.sort(h_all), rtol=4e-16, atol=0)
        keep = count > 0
        for b, (hb, vb) in zip(np.flatnonzero(keep), zip(hexp, vexp)):
            m = np.logical_and(edges[b] < h_all, h_all <= edges[b + 1])
            assert m.sum() == count[b], (s, b)
            assert abs(h_all[m].mean() - hb) <= 1e-13 * hb and abs(g_all[m].mean() - vb) <= 1e-13 * vb, (s, b)
        prng = np.random.default_rng(2020)
        spread = np.zeros(3)
        for _ in range(32):
            hp = hexp * (1 + 1e-12 * prng.uniform(-1, 1, hexp.size)); vp = vexp * (1 + 1e-12 * prng.uniform(-1, 1, vexp.size))
            rp, _, _ = va._fit_vario(hp, vp, model=va.__exponential__, x0=None, Nparm=3)
            spread = np.maximum(spread, np.abs(rp.x - res.x))
        print(f'{s}: bins {int(keep.sum())}/19, fit {res.x}, spread under 1e-12 input noise {spread} (relative {spread / np.abs(res.x)})')
        out.update({f'{s}_values': data, f'{s}_hmax': np.nanmax(dists), f'{s}_edges': edges, f'{s}_count': count, f'{s}_hexp': hexp,
                    f'{s}_vexp': vexp, f'{s}_fit': res.x, f'{s}_fit_spread': spread})
    # below the density threshold: the empty sample
    import logging
    logging.disable(logging.CRITICAL)          # (the reference's warning of this branch has a malformed format string)
    d9, i9 = va._get_samples(vals['a'][:9])
    logging.disable(logging.NOTSET)
    assert len(d9) == 0 and len(i9) == 0
    out['few_n'] = np.int64(9); out['few_samples'] = np.int64(len(d9)); out['density_threshold'] = np.int64(va.densitythreshold)
    import json
    import scipy
    from oracle.refharness import ref_import
    out['_meta'] = np.array(json.dumps(dict(ref_import.provenance(), numpy=np.__version__, scipy=scipy.__version__,
                                            # (the suite's provenance check of g*.npz asks for the family's generator by name)
                                            generator='tools/gen_golden_variogram.py, companion of oracle/refharness/gen_golden.py')))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(a.out, **out)
    print(a.out, Path(a.out).stat().st_size, 'bytes')


if __name__ == '__main__':
    main()
