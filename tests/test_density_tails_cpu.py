"""The front end's densities and element-wise functions far in their tails, on the host: the numpy evaluation of each model's graph
(tests/density_tail_models.py) against the 60-digit restatement and its bound (tests/density_tail_reference.py), the measurement of the
host's library that sets the allowances A_f, and the fixture's own checks."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import density_tail_models as M  # noqa: E402
import density_tail_reference as R  # noqa: E402


@pytest.fixture(scope="module")
def fix():
    return M.fixture()


def test_fixture_is_small_and_holds_arguments_values_and_scales_only(fix):
    assert os.path.getsize(R.FIXTURE) < 187 * 1024
    want = {f"data_{c}" for c in list(R.DATA) + ["lf", "lb"]}
    want |= {f"fn_{n}_{k}" for n in R.FUNCTIONS for k in R.COLUMNS}
    want |= {f"den_{n}_{k}" for n in R.DENSITIES for k in ("q", "value", "value_lo", "vscale", "grad", "grad_lo", "gscale")}
    assert set(fix) == want
    assert all(v.dtype == np.float64 for v in fix.values())


def test_every_grid_contains_its_named_edge_points(fix):
    for name, edges in R.EDGES.items():
        x = fix[f"fn_{name}_x"]
        assert len(x) <= 64 and np.array_equal(x, np.array(R.FUNCTIONS[name])), name
        assert set(float(e) for e in edges) <= set(x.tolist()), name
    from scipy.special import gammaln

    assert fix["data_y"].tolist() == [-1.3, 0.2, 40.0] and fix["data_pos"].tolist() == [1e-3, 1.0, 50.0]
    assert fix["data_unit"].tolist() == [1e-9, 0.5, 1.0 - 1e-9]
    assert fix["data_cnt"].tolist() == [0.0, 3.0, 50.0] and fix["data_ntr"].tolist() == [1.0, 7.0, 50.0]
    cnt, ntr = fix["data_cnt"], fix["data_ntr"]
    assert np.array_equal(fix["data_lf"], gammaln(cnt + 1.0))
    assert np.array_equal(fix["data_lb"], gammaln(ntr + 1.0) - gammaln(cnt + 1.0) - gammaln(ntr - cnt + 1.0))
    assert R.Q9 == (-30, -12, -3, 0, 3, 8, 14, 20, 25) and R.Q5 == (-12, -3, 0, 3, 8) and R.LOC == (-500, -3, 0, 40, 500)
    assert R.LOGIT == (-745, -37, -3, 0, 3, 37, 709) and R.PHI == (-12, -3, 0, 3, 5, 7, 12, 18, 25, 30) and R.ETA == (-4, 0, 3, 12)
    for name, e in R.DENSITIES.items():
        q = fix[f"den_{name}_q"]
        assert np.array_equal(q, R.grid(name)) and q.shape == (math.prod(len(g) for _, _, g in e["params"]), len(e["params"])), name
        for _, kind, g in e["params"]:      # a positive parameter runs over the wide grid unless the density overflows there
            assert g in ((R.Q9, R.PHI, R.Q5, R.Q4) if kind == "pos" else (R.LOC, R.LOGIT, R.LOG_RATE, R.ETA, (-3.0,))), name
    grid = {tuple(r) for r in fix["den_negative_binomial_log_q"].tolist()}
    assert {(0.0, 5.0), (12.0, 30.0), (-4.0, 25.0)} <= grid      # (the row y = 3, phi = e^5 among them)


def test_every_reference_value_and_gradient_is_finite(fix):
    """no row of a density may be skipped"""
    for name in R.DENSITIES:
        t = R.density_table(fix, name)
        for k, v in t.items():
            assert np.isfinite(v).all(), (name, k)
        assert (t["vscale"] >= R.N_OBS).all() and (t["gscale"] >= R.N_OBS + 1).all(), name


def test_fixture_is_what_the_reference_gives(fix):
    """a thinned subset of rows recomputed with mpmath"""
    pytest.importorskip("mpmath")
    for name in R.FUNCTIONS:
        pick = list(range(0, len(R.FUNCTIONS[name]), 7))
        t = R.function_rows(name, [R.FUNCTIONS[name][i] for i in pick])
        for k, v in t.items():
            assert np.array_equal(v, fix[f"fn_{name}_{k}"][pick], equal_nan=True), (name, k)
    data = {c: fix[f"data_{c}"] for c in list(R.DATA) + ["lf", "lb"]}
    for name in R.DENSITIES:
        n = len(fix[f"den_{name}_q"])
        pick = list(range(n % 5, n, 13))
        t = R.density_rows(name, data, pick)
        for k, v in t.items():
            assert np.array_equal(v, fix[f"den_{name}_{k}"][pick]), (name, k)


def _host(name):
    """the numpy evaluation of the function model: (value ratios, derivative ratios or None) in units of A_f = 1"""
    m, pos = M.function_model(name)
    _, g = m.logp_and_grad_numpy(pos)
    value, deriv = M.function_outputs(name, g[0])
    return R.function_ratios(name, R.table(M.fixture(), name), value, deriv)


def test_the_allowances_are_four_times_the_hosts_worst(fix):
    """A_f = max(4, 4 x the worst error of the host's library on the table, rounded up): the measurement, against what the reference
    module records (HOST_WORST) and derives from it"""
    for name in R.FUNCTIONS:
        rv, rd = _host(name)
        x = fix[f"fn_{name}_x"]
        failed = np.isinf(rv) & np.isfinite(fix[f"fn_{name}_f"])      # no finite value from the host where the exact one is finite
        assert sorted(x[failed].tolist()) == sorted(R.HOST_FAILS.get(name, ())), (name, x[failed])
        rv = np.where(failed, 0.0, rv)
        worst = (float(rv.max()), float(rd.max()) if rd is not None else 0.0)
        print(f"host {name}: value {worst[0]:.3f} at x = {x[int(rv.argmax())]!r}, derivative {worst[1]:.3f}"
              + (f" at x = {x[int(rd.argmax())]!r}" if rd is not None else "") + f", A = {R.A[name]}")
        assert worst[0] <= R.HOST_WORST[name][0] + 5e-4 and worst[1] <= R.HOST_WORST[name][1] + 5e-4, (name, worst)
        assert R.A[name] == max(4, math.ceil(4.0 * max(R.HOST_WORST[name]))), name
        assert 4.0 * max(worst) <= R.A[name], name


@pytest.mark.parametrize("name", list(R.DENSITIES))
def test_numpy_evaluation_of_every_row_is_within_the_bound(fix, name):
    """logp and every gradient element of every row within (N - 1 + c) 2^-53 scale (the gradient: 2 c) of the 60-digit value"""
    t = R.density_table(fix, name)
    lp, g = M.density_model(name).logp_and_grad_numpy(t["q"])
    rv, rg = R.density_ratios(name, t, lp, g)
    c = R.DENSITIES[name]["c"]
    units_v, units_g = rv.max() * (R.N_OBS - 1 + c), rg.max() * (R.N_OBS - 1 + 2 * c)
    print(f"{name}: {len(lp)} rows, c = {c}; value {units_v:.3g} units (err / bound {rv.max():.3g}) at q = {t['q'][int(rv.argmax())].tolist()}; "
          f"gradient {units_g:.3g} units (err / bound {rg.max():.3g}) at q = {t['q'][int(rg.max(axis=1).argmax())].tolist()}")
    R.record(f"numpy {name}", float(max(rv.max(), rg.max())))
    assert rv.max() <= 1.0 and rg.max() <= 1.0, (name, float(rv.max()), float(rg.max()))
