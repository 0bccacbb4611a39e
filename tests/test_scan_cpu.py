"""First-order linear recurrences in the symbolic IR (linear_recurrence / cumsum): the numpy evaluation against a Python loop, the
symbolic gradient against central differences and torch.autograd, the torch front end (long cumsum, the custom op), the generated
source, and cross-compilation of the device routine (csrc/chain_scan.h) at one, two and four waves per chain."""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import scan_models as sm  # noqa: E402

from nutpie_amd import symbolic as S  # noqa: E402


def _loop(a, b, init, R, T):
    """x_t = a_t x_{t-1} + b_t per row, plain Python"""
    x = np.empty((R, T))
    for r in range(R):
        prev = init[r]
        for t in range(T):
            prev = a[r, t] * prev + b[r, t]
            x[r, t] = prev
    return x


@pytest.mark.parametrize("T", [1, 63, 64, 65, 200, 4097])
@pytest.mark.parametrize("R", [1, 8])
@pytest.mark.parametrize("a_kind", ["scalar", "vector", "one"])
@pytest.mark.parametrize("init_kind", ["const", "param"])
def test_numpy_evaluation_equals_a_python_loop(T, R, a_kind, init_kind):
    if R > 1 and init_kind == "param":
        init_kind = "row"
    m = sm.scan_model(R, T, a_kind, init_kind, seed=T, deterministic=True)
    c = m.compile()
    x = sm.points(c.n_dim, 2, seed=R + T)
    names = c._front._unconstrained
    for row in x:
        def raw(name):
            _, off, n = names[name]
            return row[off:off + n]
        s = np.exp(raw("s")[0])
        b = (s * raw("z")).reshape(R, T)
        if a_kind == "one":
            a = np.ones((R, T))
        elif a_kind == "scalar":
            a = np.full((R, T), 2.0 / (1.0 + np.exp(-raw("phi")[0])) - 1.0)
        else:
            a = np.tanh(raw("av")).reshape(R, T)
        init = np.full(R, 0.25) if init_kind == "const" else (np.full(R, raw("x0")[0]) if init_kind == "param" else raw("x0r"))
        got = c._expand_func(row[None], **c._data)["path"].reshape(R, T)
        np.testing.assert_allclose(got, _loop(a, b, init, R, T), rtol=1e-12, atol=1e-14)


def _central(c, x, h=1e-6):
    g = np.zeros_like(x)
    for k in range(x.shape[1]):
        e = np.zeros(x.shape[1])
        e[k] = h
        g[:, k] = (c.logp_and_grad_numpy(x + e)[0] - c.logp_and_grad_numpy(x - e)[0]) / (2 * h)
    return g


@pytest.mark.parametrize("T", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("R", [1, 8])
@pytest.mark.parametrize("a_kind", ["scalar", "vector", "one"])
@pytest.mark.parametrize("init_kind", ["const", "param"])
def test_gradient_matches_central_differences(T, R, a_kind, init_kind):
    if R > 1 and init_kind == "param":
        init_kind = "row"
    c = sm.scan_model(R, T, a_kind, init_kind, seed=T).compile()
    x = sm.points(c.n_dim, 2, seed=7 * T + R)
    _, g = c.logp_and_grad_numpy(x)
    np.testing.assert_allclose(g, _central(c, x), rtol=1e-6, atol=1e-6 * np.abs(g).max())


def test_gradient_of_a_long_series_matches_central_differences_on_its_parameters():
    # T = 4097: the coordinates that are not per-element (s, phi, x0) — central differences over all 4 100 would take minutes
    c = sm.scan_model(1, 4097, "scalar", "param", seed=3).compile()
    x = sm.points(c.n_dim, 2, seed=5)
    _, g = c.logp_and_grad_numpy(x)
    for name in ("s", "phi", "x0"):
        _, off, _ = c._front._unconstrained[name]
        e = np.zeros(c.n_dim)
        e[off] = 1e-6
        num = (c.logp_and_grad_numpy(x + e)[0] - c.logp_and_grad_numpy(x - e)[0]) / 2e-6
        np.testing.assert_allclose(g[:, off], num, rtol=1e-6, atol=1e-5)   # (a sum of 4 097 terms: the differences carry ~1e-7 of rounding)


@pytest.mark.parametrize("example", ["sv", "garch", "ar1"])
def test_examples_match_their_torch_twins(example):
    import torch

    from nutpie_amd import timeseries as TS
    from nutpie_amd.torch_trace import trace

    make, twin = {"sv": (TS.stochastic_volatility_model, TS.stochastic_volatility_torch_density),
                  "garch": (TS.garch11_model, TS.garch11_torch_density), "ar1": (TS.ar1_latent_model, TS.ar1_latent_torch_density)}[example]
    c = make().compile()
    D, logp = twin()
    assert D == c.n_dim
    x = sm.points(D, 3, seed=1, scale=0.2)
    if example == "sv":
        x[:, 0] -= 9.0
    lp, g = c.logp_and_grad_numpy(x)
    xt = torch.tensor(x, requires_grad=True)
    lt = logp(xt)
    lt.sum().backward()
    np.testing.assert_allclose(lp, lt.detach().numpy(), rtol=1e-10)
    np.testing.assert_allclose(g, xt.grad.numpy(), rtol=1e-10, atol=1e-10 * np.abs(g).max())
    # traced (torch.cumsum of 2000 elements, the custom op): the same density, compiled to a scan stage
    ct = trace(logp, D).compile()
    assert '#include "chain_scan.h"' in ct._source
    lp2, g2 = ct.logp_and_grad_numpy(x)
    np.testing.assert_allclose(lp2, lt.detach().numpy(), rtol=1e-10)
    np.testing.assert_allclose(g2, xt.grad.numpy(), rtol=1e-10, atol=1e-10 * np.abs(g).max())


@pytest.mark.parametrize("n", [100, 3000])
@pytest.mark.parametrize("rows", [1, 3])
def test_traced_long_cumsum_compiles_and_matches_autograd(n, rows):
    import torch

    from nutpie_amd.torch_trace import trace

    D = rows * n + 1

    def logp(x):
        s = torch.exp(x[0, 0])
        walk = torch.cumsum(s * x[0, 1:].reshape(rows, n).T, dim=0)          # along the FIRST axis: moved last by the tracer
        return (-0.5 * (x * x).sum() - 0.5 * ((walk - 0.1) ** 2).sum()).reshape(1)

    c = trace(logp, D).compile()
    assert "nphip_scan::linear_recurrence<" + str(rows) + ", " + str(n) + ", nphip_scan::A_ONE" in c._source
    x = sm.points(D, 3, seed=n, scale=0.1)
    lp, g = c.logp_and_grad_numpy(x)
    xt = torch.tensor(x, requires_grad=True)
    lt = torch.cat([logp(xt[i:i + 1]) for i in range(3)])
    lt.sum().backward()
    np.testing.assert_allclose(lp, lt.detach().numpy(), rtol=1e-10)
    np.testing.assert_allclose(g, xt.grad.numpy(), rtol=1e-10, atol=1e-10 * np.abs(g).max())


def test_custom_op_eager_gradient_matches_the_sequential_autograd():
    import torch

    from nutpie_amd.torch_trace import linear_recurrence

    rng = np.random.default_rng(4)
    a = torch.tensor(rng.uniform(-0.9, 0.9, size=(3, 70)), requires_grad=True)
    b = torch.tensor(rng.normal(size=(3, 70)), requires_grad=True)
    init = torch.tensor(rng.normal(size=3), requires_grad=True)
    w = torch.tensor(rng.normal(size=(3, 70)))
    (linear_recurrence(a, b, init) * w).sum().backward()
    got = [t.grad.clone() for t in (a, b, init)]
    for t in (a, b, init):
        t.grad = None
    prev, cols = init, []
    for t in range(70):
        prev = a[:, t] * prev + b[:, t]
        cols.append(prev)
    (torch.stack(cols, -1) * w).sum().backward()
    for g_, t in zip(got, (a, b, init)):
        np.testing.assert_allclose(g_.numpy(), t.grad.numpy(), rtol=1e-12, atol=1e-13)
    # any axis: dim=0 on the transposed tensor is the same recurrence
    x1 = linear_recurrence(a.detach(), b.detach(), init.detach())
    x0 = linear_recurrence(a.detach().T, b.detach().T, init.detach(), dim=0)
    np.testing.assert_array_equal(x1.numpy(), x0.T.numpy())


def test_sources_without_scans_are_unchanged():
    import matrix_models
    import symbolic_models
    import torch_models

    from nutpie_amd import radon
    from nutpie_amd.torch_trace import trace

    def h(c):
        assert "chain_scan" not in c._source and "nphip_scan::" not in c._source
        return hashlib.sha256(c._source.encode()).hexdigest()

    assert h(radon.radon_symbolic_model().compile()) == "6733028583b22380ff8ce538d583554a3cc1b52c57c6594aeae8e21026fd21f8"
    assert h(symbolic_models.ordinal_regression().compile()) == "ac60bfde55d144bbceee07f37112ebdf7cb5fc40b2ef9fbfc666e682c98dabbf"
    assert h(matrix_models.gp_rows(3, 5).compile()) == "5a0fc5775edbb050b6b85df4dd0fa98a75dd5eb95c93ea3a8601e7778f9046ce"
    D, fn, batched, shared = torch_models.ordered_logistic()
    assert h(trace(fn, D, batched=batched, shared_data=shared).compile()) == "caa09ac7efa6a3830cc7ac6038cc519c3f377c9e819efdeb0aa9152ea7da8603"


def test_the_source_calls_the_scan_routine_forward_and_backward():
    from nutpie_amd.timeseries import stochastic_volatility_model

    src = stochastic_volatility_model().compile()._source
    assert src.count('#include "chain_scan.h"') >= 1
    assert "nphip_scan::linear_recurrence<1, 2000, nphip_scan::A_ONE, false, false>" in src
    assert "nphip_scan::linear_recurrence<1, 2000, nphip_scan::A_ONE, true, false>" in src
    assert "nphip_expand(" in src            # the volatility deterministic: generated device code


@pytest.mark.parametrize("W", [1, 2, 4])
def test_stochastic_volatility_density_compiles_for_gfx950(W):
    from nutpie_amd.density import compile_density, data_layout
    from nutpie_amd.timeseries import stochastic_volatility_model

    c = stochastic_volatility_model().compile(waves_per_chain=W)
    assert os.path.exists(compile_density(c._source, data_layout(c._data), c.n_dim, waves=W))


def test_malformed_along_is_a_value_error():
    m = S.Model()
    m.dim("row", 3)
    m.dim("time", 10)
    P = m.product("row", "time")
    z = m.param("z", dim=P.name)
    with pytest.raises(ValueError, match="outer"):
        S.linear_recurrence(0.5, z, along="row")
    with pytest.raises(ValueError, match="names no axis"):
        S.linear_recurrence(0.5, z, along="days")
    assert S.cumsum(z, along="time").payload == (3, 10)
    w = m.param("w", dim="time")
    with pytest.raises(ValueError, match="names no axis"):
        S.cumsum(w, along="row")
    with pytest.raises(ValueError):
        S.linear_recurrence(m.param("q", dim="row"), z, along="time")     # a on another dimension


def test_cumprod_still_raises():
    import torch

    from nutpie_amd.torch_trace import UnsupportedTorchOp, trace

    with pytest.raises(UnsupportedTorchOp):
        trace(lambda x: torch.cumprod(x, -1).sum(-1), 100)
