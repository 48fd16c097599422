#!/usr/bin/env python3
"""Generate tests/golden/g16_time_interp.npz by RUNNING THE REFERENCE (imported in place through oracle.refharness.ref_import).

A generator: it runs only where the reference is present; no test calls it.  Re-run with
    python tools/gen_golden_time_interp.py

What it holds (data only: inputs and the reference's answers):
  nw_*   utilFcns.get_nearest_wmtimes for steps of 1, 3 and 6 h on query times within and outside the threshold of a model time,
         across midnight and exactly on a model time; cli.raider.get_weights_time_interp on every case that gives two times
  gw_*   cli.raider.getWeatherFile's decision for every (method, number of files, number of times) its seven cases distinguish:
         'file0' (the first file), 'combine' (combine_weather_files was called), 'none', or the name of the exception
  fn_*   the file names combine_weather_files gives its product (cli/raider.py:824-830)

Route taken for the cli functions: `RAiDER.utilFcns` imports through the harness.  `RAiDER.cli.raider` does not: with an empty
stand-in registered for `h5py`, its import of RAiDER.aria.calcGUNW stops at `import netCDF4`, which is not installed either.  Instead
of pinning the three cli functions on the two loose known answers of the reference's test/test_temporal_interpolate.py alone, this
tool RUNS them: it reads getWeatherFile, combine_weather_files and get_weights_time_interp out of the reference's
tools/RAiDER/cli/raider.py with `ast`, in place, and executes exactly those definitions in a namespace that holds what they name
(the reference's own get_dt, logger and exceptions; numpy; an `xr` whose open_dataset returns a small object with the `datetime`
attribute and zero fields and whose to_netcdf records the name - the arithmetic of the combination is pinned elsewhere, golden g11
and g12).  The two known answers of test_temporal_interpolate.py are kept too, as data (ka_*): 13:30 between 12:00 and 15:00 is
the mean of the two epochs (:22-70); 12:05 weighs them by np.average(weights=1/[300 s, 10500 s]) to np.allclose (:82-146).
"""
import datetime as dt
import json
import sys
import warnings
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from oracle.refharness import ref_import  # noqa: E402

ref_import.import_reference()
import ast  # noqa: E402
import types  # noqa: E402

import RAiDER.utilFcns as ref_util  # noqa: E402
from RAiDER.logger import logger as ref_logger  # noqa: E402
from RAiDER.models import customExceptions as ref_exc  # noqa: E402
from RAiDER.utilFcns import get_nearest_wmtimes  # noqa: E402


def cli_functions():
    """getWeatherFile, combine_weather_files, get_weights_time_interp as the reference's cli/raider.py defines them, executed in place"""
    src = (ref_import.REF_PKG / 'cli' / 'raider.py').read_text()
    want = ('getWeatherFile', 'combine_weather_files', 'get_weights_time_interp')
    tree = ast.parse(src)
    tree.body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in want]
    assert sorted(n.name for n in tree.body) == sorted(want)
    env = dict(np=np, dt=dt, Path=Path, Optional=None, TimeInterpolationMethod=str, logger=ref_logger, get_dt=ref_util.get_dt,
               xr=types.SimpleNamespace(open_dataset=None, Dataset=object), WrongNumberOfFiles=ref_exc.WrongNumberOfFiles,
               NoWeatherModelData=ref_exc.NoWeatherModelData, __name__='RAiDER.cli.raider', __annotations__={})
    exec(compile('from __future__ import annotations\n', '<future>', 'exec'), env)
    exec(compile(tree, str(ref_import.REF_PKG / 'cli' / 'raider.py'), 'exec', flags=__import__('__future__').annotations.compiler_flag), env)
    return env


_env = cli_functions()


class _Cli:
    """attribute view of the executed namespace: assigning cli.x rebinds the global the reference's functions see"""
    def __getattr__(self, k):
        return _env[k]

    def __setattr__(self, k, v):
        _env[k] = v


cli = _Cli()

GOLD = REPO / 'tests' / 'golden'
EPOCH = dt.datetime(2020, 1, 1)
secs = lambda t: (t - EPOCH).total_seconds()


def nearest_times(out):
    queries = [dt.datetime(2020, 1, 1, 11, 35, 0),            # the docstring example
               dt.datetime(2020, 1, 1, 11, 59, 30), dt.datetime(2020, 1, 1, 12, 0, 59), dt.datetime(2020, 1, 1, 12, 1, 0),
               dt.datetime(2020, 1, 1, 12, 4, 0), dt.datetime(2020, 1, 1, 12, 6, 0), dt.datetime(2020, 1, 1, 11, 55, 0),
               dt.datetime(2020, 1, 1, 12, 0, 0), dt.datetime(2020, 1, 1, 0, 0, 0),                          # exact model times
               dt.datetime(2020, 1, 1, 23, 40, 0), dt.datetime(2020, 1, 2, 0, 20, 0), dt.datetime(2020, 1, 1, 22, 10, 0),   # across midnight
               dt.datetime(2020, 1, 1, 13, 30, 0), dt.datetime(2020, 1, 1, 14, 59, 59), dt.datetime(2020, 1, 1, 9, 0, 0, 500000),
               dt.datetime(2020, 1, 24, 13, 52, 44), dt.datetime(2020, 1, 24, 13, 52, 44, 250000)]
    q, step, n, t1, t2, w1, w2 = [], [], [], [], [], [], []
    for s in (1, 3, 6):
        for t0 in queries:
            got = get_nearest_wmtimes(t0, s)
            q.append(secs(t0)); step.append(s); n.append(len(got))
            t1.append(secs(got[0])); t2.append(secs(got[-1]))
            if len(got) == 2:
                w = cli.get_weights_time_interp(got, t0)
                w1.append(w[0]); w2.append(w[1])
            else:
                w1.append(np.nan); w2.append(np.nan)
    out['nw_query_s'], out['nw_step_h'], out['nw_n'] = np.array(q), np.array(step), np.array(n)
    out['nw_t1_s'], out['nw_t2_s'], out['nw_w1'], out['nw_w2'] = np.array(t1), np.array(t2), np.array(w1), np.array(w2)
    print(f'  get_nearest_wmtimes: {len(q)} cases, {int((np.array(n) == 1).sum())} with one time')


def weather_file_cases(out):
    files = [Path(f'/data/weather_files/HRRR_2020_01_01_T{h:02d}_00_00_32N_36N_121W_114W.nc') for h in (12, 13, 11)]
    called = []
    orig = cli.combine_weather_files
    cli.combine_weather_files = lambda wfiles, time, model, interp_method='center_time': called.append(interp_method) or 'combined'
    rows = []
    try:
        for method in ('none', 'center_time', 'azimuth_time_grid', 'nearest'):
            for nfiles in range(0, 4):
                for ntimes in range(1, 4):
                    called.clear()
                    try:
                        got = cli.getWeatherFile(files[:nfiles], list(range(ntimes)), dt.datetime(2020, 1, 1, 12, 20), 'HRRR', method)
                        verdict = 'none' if got is None else 'combine' if got == 'combined' else 'file0'
                        assert verdict != 'file0' or got == files[0]
                    except Exception as exc:
                        verdict = type(exc).__name__
                    rows.append((method, nfiles, ntimes, verdict))
    finally:
        cli.combine_weather_files = orig
    out['gw_method'] = np.array([r[0] for r in rows]); out['gw_nfiles'] = np.array([r[1] for r in rows])
    out['gw_ntimes'] = np.array([r[2] for r in rows]); out['gw_verdict'] = np.array([r[3] for r in rows])
    print('  getWeatherFile:', len(rows), 'cases;', sorted(set(r[3] for r in rows)))


def file_names(out):
    class Fields(dict):
        attrs = None

        def __getitem__(self, k):
            return 0.0

        def __setitem__(self, k, v):
            pass

        def to_netcdf(self, path):
            written.append(Path(path))

    written = []
    stamps = {}

    def open_dataset(f):
        ds = Fields(); ds.attrs = {'datetime': stamps[str(f)]}
        return ds
    orig = cli.xr.open_dataset
    cli.xr.open_dataset = open_dataset
    cases = [('GMAO_2020_01_24_T12_00_00_32N_36N_121W_114W.nc', 'GMAO_2020_01_24_T15_00_00_32N_36N_121W_114W.nc', dt.datetime(2020, 1, 24, 13, 52, 44)),
             ('ERA-5_2019_11_17_T20_00_00_5S_2S_41W_37W.nc', 'ERA-5_2019_11_17_T21_00_00_5S_2S_41W_37W.nc', dt.datetime(2019, 11, 17, 20, 51, 58)),
             ('HRRR_2021_12_31_T23_00_00_32N_36N_121W_114W.nc', 'HRRR_2022_01_01_T00_00_00_32N_36N_121W_114W.nc', dt.datetime(2021, 12, 31, 23, 59, 1))]
    first, query, name = [], [], []
    try:
        for a, b, t in cases:
            pa, pb = Path('/data/wm') / a, Path('/data/wm') / b
            for p in (pa, pb):
                stem = p.name.split('_T')[0].split('_', 1)[1] + 'T' + p.name.split('_T')[1][:8]
                stamps[str(p)] = stem
            got = cli.combine_weather_files([pa, pb], t, a.split('_')[0], interp_method='center_time')
            assert got == written[-1] and got.parent == pa.parent
            first.append(a); query.append(secs(t)); name.append(got.name)
    finally:
        cli.xr.open_dataset = orig
    out['fn_first'], out['fn_query_s'], out['fn_name'] = np.array(first), np.array(query), np.array(name)
    out['fn_style_azimuth'] = np.array('_timeInterpAziGrid_')          # STYLE['azimuth_time_grid'] (cli/raider.py:794), used by the same expression
    print('  names:', name)


def known_answers(out):
    # test/test_temporal_interpolate.py, as data: (t1, t2, query) in seconds since the epoch, and what the test expects of the weights
    d = dt.datetime(2020, 1, 30)
    out['ka_t1_s'] = np.array([secs(d.replace(hour=12)), secs(d.replace(hour=12))])
    out['ka_t2_s'] = np.array([secs(d.replace(hour=15)), secs(d.replace(hour=15))])
    out['ka_query_s'] = np.array([secs(d.replace(hour=13, minute=30)), secs(d.replace(hour=12, minute=5))])
    out['ka_w1'] = np.array([0.5, (1 / 300) / (1 / 300 + 1 / 10500)])          # the mean; np.average(weights=1 / [300, 10500])
    out['ka_allclose'] = np.array([0, 1])                                       # the second is asserted with np.allclose on delays only


def main():
    warnings.filterwarnings('ignore')
    out = {'epoch': np.array(EPOCH.isoformat())}
    nearest_times(out)
    weather_file_cases(out)
    file_names(out)
    known_answers(out)
    out['_meta'] = np.array(json.dumps(dict(ref_import.provenance(), numpy=np.__version__,
                                            # (the suite's provenance check of g*.npz asks for the family's generator by name)
                                            generator='tools/gen_golden_time_interp.py, companion of oracle/refharness/gen_golden.py')))
    path = GOLD / 'g16_time_interp.npz'
    np.savez_compressed(path, **out)
    print(f'g16_time_interp: {path.stat().st_size / 1024:.1f} KiB  keys={list(out)}')


if __name__ == '__main__':
    main()
