"""The variogram-fit contract (include/raider_hip.h: rdr_variogram_fit) as tests/variogram_fit_model.py restates it, on the CPU.

The 21 golden rows are the fit inputs that g20 (a, b, c) and g21 (four total rows, fourteen slices) record.  On every one of them the
reference's optimiser - scipy.optimize.least_squares as fit_variogram runs it - stops above the minimum of its own objective over its own
box: its cost is 1.00086 to 1.66 times the model's (measured; the smallest margin is 0.086 %).  The model may not lose to it."""
import numpy as np
import pytest

from raider_amd import variogram as V
from tests import variogram_fit_model as M

EPS = 2.0 ** -52


def test_the_model_never_loses_to_scipy_on_the_golden_rows():
    names, h, g, recorded = M.golden_rows()
    assert len(names) == 21 and h.shape == (21, 19)
    fit = M.golden_fits()
    assert (fit['status'] == 0).all()
    worst = np.inf
    for i, name in enumerate(names):
        keep = ~np.isnan(h[i])
        res = V.fit_variogram(h[i][keep], g[i][keep]).result
        assert fit['cost'][i] <= res.cost * (1 + 1e-9), (name, fit['cost'][i], res.cost)
        worst = min(worst, res.cost / fit['cost'][i])
        if not np.isnan(recorded[i, 0]):
            at_recorded = M.cost_at(h[i], g[i], recorded[i, 0], recorded[i, 1])
            assert fit['cost'][i] <= at_recorded, (name, fit['cost'][i], at_recorded)
            assert fit['params'][i, 2] == 0.4 * np.nanmax(g[i]) == recorded[i, 2]              # the nugget start comes back untouched
    print(f'smallest scipy cost / model cost over the golden rows: {worst:.6f}')
    assert worst > 1.0


def test_a_scan_of_512_reaches_the_cost_of_8192():
    """within the float64-against-long-double spread of the cost (x 16, floor 32 eps relative)"""
    f64, ld, fine = M.golden_fits(), M.golden_fits(np.longdouble), M.golden_fits(np.float64, 8192)
    spread = np.max(np.abs(f64['cost'] - ld['cost']) / ld['cost']).astype(np.float64)
    gap = np.max(np.abs(f64['cost'] - fine['cost']) / fine['cost'])
    print(f'cost: float64 / long double spread {spread:.2e}, K = 512 against K = 8192 {gap:.2e}')
    assert gap <= max(16 * spread, 32 * EPS)


def test_the_range_is_determined_off_the_plateau():
    """the rows the GPU test may leave out of its range check (float64 and long double ranges apart by more than 1e-6) are at most 20 %"""
    f64, ld = M.golden_fits(), M.golden_fits(np.longdouble)
    apart = np.abs(f64['params'][:, 0] - ld['params'][:, 0]) > 1e-6 * ld['params'][:, 0]
    assert apart.mean() <= 0.2, apart
    assert np.array_equal(f64['flags'], ld['flags'])


@pytest.mark.parametrize('a0, b0', M.EXACT)
def test_exact_exponentials_are_recovered(a0, b0):
    h, g, ub = M.exact_row(a0, b0)
    fit = M.fit_row(h, g, ub=ub)
    assert fit['status'] == 0 and fit['flags'] == 0
    assert abs(fit['params'][0] - a0) <= 1e-9 * a0 and abs(fit['params'][1] - b0) <= 1e-9 * b0, fit['params']


def test_status_rows():
    nan = np.nan
    h = np.array([1000.0, 2000.0, 3000.0]); g = np.array([1e-4, 2e-4, 2.5e-4])
    assert M.fit_row([nan, nan, 3.0], [1.0, nan, nan])['status'] == 1
    assert M.fit_row(h, -g)['status'] == 2
    assert M.fit_row([0.0, 0.0, nan], g)['status'] == 3
    assert M.fit_row([-1.0, 2000.0, 3000.0], g)['status'] == 2
    assert M.fit_row(h, [1e-4, np.inf, 2e-4])['status'] == 2
    assert M.fit_row(h, g, ub=[0.0, 1.0, 1.0])['status'] == 2
    fit = M.fit_row(h, [1e-5, -1e-4, -3e-4])
    assert fit['status'] == 0 and fit['params'][1] == 0 and fit['flags'] == M.SILL_ZERO | M.AT_FLOOR
