"""The models the density-tail tests run (tests/test_density_tails_cpu.py, tests/test_gpu_density_tails.py): one ``Model`` per density
entry of tests/density_tail_reference.py — ``add_logp(density(...).sum())`` over the three observations, the parameters in the entry's
order — and one per function of its table: parameters x[n] and c[n], logp = (c f(x)).sum().  At c = 1 the gradient in c_i is f(x_i) and
the gradient in x_i the derivative rule's value, both exact products with 1.0: one ``logp_and_grad`` returns the value and the derivative
at every argument of the table.  digamma has no derivative rule: its x is data.

Data columns, arguments and positions come from the fixture (tests/golden/density_tail_reference.npz), which is all a GPU machine needs.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import density_tail_reference as R  # noqa: E402

import nutpie_amd.symbolic as S  # noqa: E402

_FIX = None


def fixture():
    global _FIX
    if _FIX is None:
        with np.load(R.FIXTURE) as z:
            _FIX = {k: z[k] for k in z.files}
    return _FIX


#: name -> the front end's density of (data columns d, parameters p in the entry's order)
_BUILD = {
    "normal": lambda d, p: S.normal_lpdf(d["y"], p[0], p[1]),
    "halfnormal": lambda d, p: S.halfnormal_lpdf(d["pos"], p[0]),
    "student_t_number": lambda d, p: S.student_t_lpdf(d["y"], 3.5, p[0], p[1]),
    "student_t_expr": lambda d, p: S.student_t_lpdf(d["y"], p[0] + 1.0, p[1], p[2]),
    "cauchy": lambda d, p: S.cauchy_lpdf(d["y"], p[0], p[1]),
    "halfcauchy": lambda d, p: S.halfcauchy_lpdf(d["pos"], p[0]),
    "exponential": lambda d, p: S.exponential_lpdf(d["pos"], p[0]),
    "lognormal": lambda d, p: S.lognormal_lpdf(d["pos"], p[0], p[1]),
    "gamma": lambda d, p: S.gamma_lpdf(d["pos"], p[0], p[1]),
    "inverse_gamma": lambda d, p: S.inverse_gamma_lpdf(d["pos"], p[0], p[1]),
    "beta": lambda d, p: S.beta_lpdf(d["unit"], p[0], p[1]),
    "laplace": lambda d, p: S.laplace_lpdf(d["y"], p[0], p[1]),
    "logistic": lambda d, p: S.logistic_lpdf(d["y"], p[0], p[1]),
    "weibull": lambda d, p: S.weibull_lpdf(d["pos"], p[0], p[1]),
    "bernoulli_logit": lambda d, p: S.bernoulli_logit_lpmf(d["bin"], p[0]),
    "binomial_logit": lambda d, p: S.binomial_logit_lpmf(d["cnt"], d["ntr"], p[0], d["lb"]),
    "poisson_log": lambda d, p: S.poisson_log_lpmf(d["cnt"], p[0], d["lf"]),
    "negative_binomial_log": lambda d, p: S.negative_binomial_log_lpmf(d["cnt"], p[0], p[1], d["lf"]),
}
assert set(_BUILD) == set(R.DENSITIES)
_FN = {name: getattr(S, name) for name in R.FUNCTIONS}
_MODELS = {}


def density_model(name: str):
    """the compiled model of the density entry ``name`` (cached per process); its positions are ``fixture()["den_<name>_q"]``"""
    key = ("den", name)
    if key not in _MODELS:
        e, fix = R.DENSITIES[name], fixture()
        m = S.Model()
        p = [m.param(pn, lower=0.0 if kind == "pos" else None) for pn, kind, _ in e["params"]]
        d = {col: m.data(col, fix[f"data_{col}"], dim="obs") for col in e["data"]}
        m.add_logp(_BUILD[name](d, p).sum())
        _MODELS[key] = m.compile()
    return _MODELS[key]


def function_model(name: str):
    """the compiled model of the function ``name``: (model, the position [1, D] that holds the table's arguments and c = 1)"""
    key = ("fn", name)
    if key not in _MODELS:
        x = fixture()[f"fn_{name}_x"]
        n = len(x)
        m = S.Model()
        if name in R.NO_DERIVATIVE:
            c = m.param("c", dim="pt", size=n)
            m.add_logp((c * _FN[name](m.data("x", x, dim="pt"))).sum())
            pos = np.ones((1, n))
        else:
            xp = m.param("x", dim="pt", size=n)
            c = m.param("c", dim="pt", size=n)
            m.add_logp((c * _FN[name](xp)).sum())
            pos = np.concatenate([x, np.ones(n)])[None, :]
        _MODELS[key] = (m.compile(), pos)
    return _MODELS[key]


def function_outputs(name: str, grad):
    """(values, derivatives or None) per argument from the gradient [D] of ``function_model(name)`` at its position"""
    n = len(fixture()[f"fn_{name}_x"])
    if name in R.NO_DERIVATIVE:
        return grad[:n], None
    return grad[n:2 * n], grad[:n]


def all_models():
    return [density_model(name) for name in R.DENSITIES] + [function_model(name)[0] for name in R.FUNCTIONS]
