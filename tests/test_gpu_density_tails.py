"""The front end's element-wise functions and densities on the GPU, far in their tails (tests/density_tail_models.py): every function
value and derivative of the table within its allowance A_f, every density row within the bound that tests/density_tail_reference.py
derives from a 60-digit restatement, overflow rows equal to the expected infinity, a poisoned chain contained.  One launch per model;
the libraries are prebuilt (tests/prebuild_density_tail_cache.py); only the fixture is read."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import density_tail_models as M  # noqa: E402
import density_tail_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _device(name):
    m, pos = M.function_model(name)
    _, g = m.logp_and_grad(pos)
    return M.function_outputs(name, g[0])


@pytest.mark.parametrize("name", list(R.FUNCTIONS))
def test_every_function_value_and_derivative_is_within_its_allowance(hip, name):
    """in units of 2^-53 (|f| + |x f'|) and 2^-53 (|f'| + |x f''|): at most A_f, an expected-limit row (``R.LIMITS``) at most its limit"""
    t = R.table(M.fixture(), name)
    value, deriv = _device(name)
    rv, rd = R.function_ratios(name, t, value, deriv)
    failed = []
    for what, r, got, want in (("value", rv, value, t["f"]), ("derivative", rd, deriv, t["d"])):
        if r is None:
            continue
        allowed = np.array([R.LIMITS.get((name, what), {}).get(float(x), (R.A[name],))[0] for x in t["x"]], dtype=np.float64)
        i = int(np.argmax(r / allowed))
        R.record(f"device {name} {what}: {r[i]:.3f} units of A = {allowed[i]:g} at x = {t['x'][i]!r}", float(r[i] / allowed[i]))
        for j in np.flatnonzero(~(r <= allowed)):
            failed.append((what, float(t["x"][j]), float(got[j]), float(want[j]), float(r[j])))
    assert not failed, failed


def test_overflow_rows_are_the_expected_infinity(hip):
    seen = 0
    for name in R.FUNCTIONS:
        t = R.table(M.fixture(), name)
        value, deriv = _device(name)
        over = np.isinf(t["f"])
        assert np.array_equal(value[over], t["f"][over]), (name, t["x"][over], value[over])
        seen += int(over.sum())
        if deriv is not None:
            over = np.isinf(t["d"])
            assert np.array_equal(deriv[over], t["d"][over]), (name, t["x"][over], deriv[over])
            seen += int(over.sum())
    assert seen >= 8      # exp, expm1 past 709.78 (value and derivative), lgamma past 2.55e305, lgamma' at the smallest subnormal


@pytest.mark.parametrize("name", list(R.DENSITIES))
def test_every_density_row_is_within_the_bound(hip, name):
    """one launch, a chain per row of the grid: logp within (N - 1 + c) 2^-53 scale, every gradient element within (N - 1 + 2 c) 2^-53 scale"""
    t = R.density_table(M.fixture(), name)
    lp, g = M.density_model(name).logp_and_grad(t["q"])
    rv, rg = R.density_ratios(name, t, lp, g)
    print(f"{name}: value err / bound {rv.max():.3g} at q = {t['q'][int(rv.argmax())].tolist()}, "
          f"gradient {rg.max():.3g} at q = {t['q'][int(rg.max(axis=1).argmax())].tolist()}")
    R.record(f"device {name}", float(max(rv.max(), rg.max())))
    assert rv.max() <= 1.0 and rg.max() <= 1.0, (name, float(rv.max()), float(rg.max()))


@pytest.mark.parametrize("name", list(R.DENSITIES) + list(R.FUNCTIONS))
def test_a_nan_in_one_chain_leaves_the_others_their_bits(hip, name):
    """five chains, a NaN in the first coordinate of the third one's position"""
    if name in R.DENSITIES:
        m, q = M.density_model(name), M.fixture()[f"den_{name}_q"]
        pos = q[np.linspace(0, len(q) - 1, 5).astype(int)]
    else:
        m, one = M.function_model(name)
        pos = np.repeat(one, 5, axis=0)
    clean_lp, clean_g = m.logp_and_grad(pos)
    bad = pos.copy()
    bad[2, 0] = np.nan
    lp, g = m.logp_and_grad(bad)
    others = [0, 1, 3, 4]
    assert np.array_equal(_bits(lp[others]), _bits(clean_lp[others])) and np.array_equal(_bits(g[others]), _bits(clean_g[others])), name
    assert np.isnan(lp[2]) or np.isnan(g[2]).any(), name
