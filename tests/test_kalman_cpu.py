"""Linear Gaussian state-space models in the symbolic IR (nutpie_amd/symbolic.py: kalman_marginal_lpdf, kalman_filtered_state), the torch
front end (nutpie_amd/torch_trace.py: kalman_marginal) and the plain-C restatement of the device routines' order contract
(tests/fixtures/kalman_reference.c) — everything that needs no GPU.  DESIGN.md §11.9."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import kalman_models  # noqa: E402
import kalman_reference as K  # noqa: E402

from nutpie_amd import symbolic as S  # noqa: E402


# --------------------------------------------------------------------------- helpers
def ir_kalman(R, T, m, free=False, masked=False, values=None):
    """a Model whose density is kalman_marginal_lpdf of R series; the operands are data, or (``free``) unconstrained parameters
    ``[y (R T), Z (R T m), h (R T), Tm (m m), Q (m m), a0 (m), P0 (m m)]``; the mask is data.  Returns (model, keyword arguments)."""
    mod = S.Model()
    mod.dim("state", m)
    mod.dim("time", T)
    if R == 1:
        steps, along = "time", None
    else:
        mod.dim("series", R)
        steps, along = mod.product("series", "time").name, "time"
    zd, kk = mod.product(steps, "state"), mod.product("state", "state")
    dims = [steps, zd.name, steps, kk.name, kk.name, "state", kk.name]
    names = ["y", "Z", "h", "Tm", "Q", "a0", "P0"]
    if free:
        ops = [mod.param(n, dim=d) for n, d in zip(names, dims)]
    else:
        ops = [mod.data(n, np.reshape(v, -1), dim=d) for n, d, v in zip(names, dims, [values[k] for k in (0, 2, 3, 4, 5, 6, 7)])]
        mod.param("unused")
    kw = dict(design=ops[1], obs_var=ops[2], transition=ops[3], state_cov=ops[4], init_mean=ops[5], init_cov=ops[6], along=along)
    if masked:
        kw["observed"] = mod.data("observed", np.reshape(values[1], -1), dim=steps)
    mod.add_logp(S.kalman_marginal_lpdf(ops[0], **kw))
    return mod, ops[0], kw


def ir_value(R, T, m, values, masked):
    mod, *_ = ir_kalman(R, T, m, masked=masked, values=values)
    return S.evaluate([mod.logp_expr()], np.zeros((1, 1)), mod._data)[0][0]


def dense_value(y, obs, Z, h, Tm, Q, a0, P0):
    """the log density of the observed y under the joint Gaussian with the unrolled mean and covariance (scipy), summed over series"""
    from scipy.stats import multivariate_normal

    R, T = y.shape
    m = a0.size
    V, power = [P0], [np.eye(m)]
    for t in range(1, T):
        V.append(Tm @ V[-1] @ Tm.T + Q)
        power.append(Tm @ power[-1])
    total = 0.0
    for r in range(R):
        mean = np.array([Z[r, t] @ power[t] @ a0 for t in range(T)])
        cov = np.empty((T, T))
        for s in range(T):
            for t in range(s, T):
                cov[s, t] = cov[t, s] = Z[r, s] @ V[s] @ np.linalg.matrix_power(Tm.T, t - s) @ Z[r, t]
            cov[s, s] += h[r, s]
        keep = obs[r] != 0
        if keep.any():
            total += multivariate_normal(mean[keep], cov[np.ix_(keep, keep)], allow_singular=False).logpdf(y[r, keep])
    return total


def packs(values, masked, vbar, Fbar, dtype=np.float64):
    """(F, B) by the plain algorithm (S._np_kalman) in ``dtype``"""
    y, obs, Z, h, Tm, Q, a0, P0 = (np.asarray(v, dtype=dtype) for v in values)
    R, T = y.shape
    m = a0.size
    row = lambda v: np.reshape(np.asarray(v, dtype=dtype), (1, -1))      # noqa: E731
    extra = [row(obs)] if masked else []
    F = S._np_kalman("kalman_fwd", [row(v) for v in (y, Z, h, Tm, Q, a0, P0)] + extra, R, T, m, masked, 1)
    B = S._np_kalman("kalman_bwd", [row(v) for v in (y, Z, h, Tm, Q)] + [F, row(vbar), row(Fbar)] + extra, R, T, m, masked, 1)
    return F[0], B[0]


def arrays(R, T, m, F, B):
    """the named arrays of the two packs (the per-series partials are not among them: the sums are)"""
    rt = R * T
    f = np.split(F, np.cumsum([rt * m, rt * m * m, rt * m, rt]))
    b = np.split(B, np.cumsum([rt, rt, rt * m, m * m, m * m, m, m * m]))[:7]
    return dict(zip(["apred", "Ppred", "afilt", "v", "F", "ybar", "hbar", "Zbar", "Tbar", "Qbar", "a0bar", "P0bar"], f + b))


# --------------------------------------------------------------------------- 1. value
@pytest.mark.parametrize("R,T,m", [(1, 1, 1), (1, 4, 2), (3, 5, 1), (2, 6, 3), (1, 7, 4)])
@pytest.mark.parametrize("masked", [False, True])
def test_value_is_the_dense_joint_gaussian(R, T, m, masked):
    values = K.inputs(R, T, m, seed=R + 10 * T + 100 * m, missing=0.3)
    got = ir_value(R, T, m, values, masked)
    y, obs, *rest = values
    want = dense_value(y, obs if masked else np.ones_like(obs), *rest)
    assert abs(got - want) <= 1e-11 * abs(want), (got, want)


# --------------------------------------------------------------------------- 2. masking
@pytest.mark.parametrize("R,T,m,k", [(1, 9, 2, 3), (3, 6, 3, 1), (2, 5, 1, 5)])
def test_masking_the_last_steps_is_the_shorter_series(R, T, m, k):
    values = list(K.inputs(R, T, m, seed=4))
    obs = np.ones((R, T))
    obs[:, T - k:] = 0.0
    values[1] = obs
    got = ir_value(R, T, m, values, True)
    if k == T:
        assert got == 0.0
        return
    y, _, Z, h, *rest = values
    short = (y[:, :T - k], obs[:, :T - k], Z[:, :T - k], h[:, :T - k], *rest)
    want = ir_value(R, T - k, m, short, False)
    assert abs(got - want) <= 1e-14 * abs(want), (got, want)


def test_a_mask_of_ones_has_the_bits_of_no_mask():
    R, T, m = 2, 11, 3
    values = list(K.inputs(R, T, m, seed=9))
    values[1] = np.ones((R, T))
    rng = np.random.default_rng(0)
    vbar, Fbar = rng.normal(size=(R, T)), rng.normal(size=(R, T))
    for a, b in zip(packs(values, True, vbar, Fbar), packs(values, False, vbar, Fbar)):
        np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64))


# --------------------------------------------------------------------------- 3. gradient
def torch_reference(values, masked):
    """value and gradients by torch.autograd of a plain filter loop in matrix form (an implementation of its own)"""
    import torch

    y, Z, h, Tm, Q, a0, P0 = (torch.tensor(values[k], requires_grad=True) for k in (0, 2, 3, 4, 5, 6, 7))
    obs = torch.tensor(values[1]) if masked else torch.ones_like(y)
    R, T = y.shape
    total = torch.zeros((), dtype=torch.float64)
    for r in range(R):
        a, P = a0, P0
        for t in range(T):
            if obs[r, t] != 0:
                z = Z[r, t]
                v = y[r, t] - z @ a
                F = h[r, t] + z @ P @ z
                total = total - 0.5 * (np.log(2.0 * np.pi) + torch.log(F) + v * v / F)
                gain = P @ z / F
                a = a + gain * v
                P = P - torch.outer(gain, z @ P.T)
            a, P = Tm @ a, Tm @ P @ Tm.T + Q
    total.backward()
    grads = [v.grad.numpy() if v.grad is not None else np.zeros(v.shape) for v in (y, Z, h, Tm, Q, a0, P0)]
    return float(total.detach()), np.concatenate([g.reshape(-1) for g in grads]), [g.size for g in grads]


@pytest.mark.parametrize("m,T", [(1, 3), (2, 20), (4, 65), (8, 64), (3, 200)])
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("masked", [False, True])
def test_gradient_equals_autograd_of_a_plain_filter_loop(R, m, T, masked):
    """The IR gradient (numpy evaluation) with respect to every operand against torch.autograd of an independent loop: 1e-12 of the
    largest element of each operand's gradient (the figure of the sibling stages).  Note P - K M^T with M = P z (the stage) and
    P - K (z^T P^T) (the loop) are the same function of a P that is not symmetric, so the adjoints of Q and P0 agree element by element."""
    values = K.inputs(R, T, m, seed=7 * m + T + R)
    mod, *_ = ir_kalman(R, T, m, free=True, masked=masked, values=values)
    x = np.concatenate([np.reshape(values[k], -1) for k in (0, 2, 3, 4, 5, 6, 7)])[None]
    lp, g = mod.compile().logp_and_grad_numpy(x)
    value, want, lengths = torch_reference(values, masked)
    assert abs(lp[0] - value) <= 1e-12 * abs(value)
    for name, got_, want_ in zip(["y", "Z", "h", "Tm", "Q", "a0", "P0"], np.split(g[0], np.cumsum(lengths)[:-1]), np.split(want, np.cumsum(lengths)[:-1])):
        err, top = np.abs(got_ - want_).max(), np.abs(want_).max()
        assert err <= 1e-12 * max(top, 1e-300), (name, err, top)
    if T == 1:
        assert not g[0, sum(lengths[:3]):sum(lengths[:5])].any()


def test_filtered_state_and_second_derivatives_are_refused():
    mod, y, kw = ir_kalman(1, 4, 2, free=True)
    state = S.kalman_filtered_state(y, **kw)
    assert state.dim is mod._dims["time_x_state"]
    with pytest.raises(NotImplementedError):
        S.gradient(state.sum(), mod._params)
    with pytest.raises(NotImplementedError):
        S.gradient(S.kalman_filtered_state(y, predicted=True, **kw).sum(), mod._params)
    g = S.gradient(mod.logp_expr(), mod._params)
    with pytest.raises(NotImplementedError):
        S.gradient(g[3].sum(), mod._params)


# --------------------------------------------------------------------------- 4. the C restatement
SHAPES = [(1, 3), (2, 20), (4, 65), (8, 200), (3, 500)]      # (m, T), three series each, 15 % of the steps missing


def c_packs(values, masked, vbar, Fbar):
    y, obs, Z, h, Tm, Q, a0, P0 = values
    R, T = y.shape
    m = a0.size
    ob = obs if masked else None
    F = K.forward(y, ob, Z, h, Tm, Q, a0, P0, R, T, m)
    return F, K.backward(y, ob, Z, h, Tm, Q, F, vbar, Fbar, R, T, m)[:K.sizes(R, T, m)[1]]


def adjoint_seeds(values, masked):
    """vbar = -v / F and Fbar = -(1 / F - v^2 / F^2) / 2 on the observed steps: those of the density"""
    F, _ = c_packs(values, masked, np.zeros_like(values[0]), np.zeros_like(values[0]))
    R, T = values[0].shape
    m = values[6].size
    v, Fv = (a.reshape(R, T) for a in np.split(F, np.cumsum([R * T * (2 * m + m * m), R * T]))[1:])
    seen = values[1] != 0 if masked else np.ones((R, T), bool)
    return np.where(seen, -v / Fv, 0.0), np.where(seen, -0.5 * (1.0 / Fv - v * v / (Fv * Fv)), 0.0)


@pytest.mark.parametrize("m,T", SHAPES)
def test_c_restatement_equals_the_numpy_evaluation(m, T):
    """every packed array of both stages: 1e-13 of the array's largest element"""
    R = 3
    values = K.inputs(R, T, m, seed=31 * m + T)
    for masked in (False, True):
        vbar, Fbar = adjoint_seeds(values, masked)
        want = arrays(R, T, m, *packs(values, masked, vbar, Fbar))
        got = arrays(R, T, m, *c_packs(values, masked, vbar, Fbar))
        for name in want:
            err, top = np.abs(got[name] - want[name]).max(), np.abs(want[name]).max()
            assert err <= 1e-13 * top, (name, masked, err, top)


def test_c_restatement_against_long_double():
    """Both float64 evaluations against the plain algorithm in long double (64-bit mantissa), per array relative to the array's
    largest element, over the five shapes with 15 % of the steps missing.  The bound is measured, not fixed: 4 x the largest such
    error of the float64 numpy evaluation on the same inputs (the rule of the HMM test: both are O(T m u) algorithms with different
    constants).  Measured: numpy evaluation 9.72e-16, so the bound is 3.89e-15; the restatement's largest error is 8.40e-16."""
    assert np.finfo(np.longdouble).nmant >= 63
    R = 3
    worst_plain = worst_c = 0.0
    for m, T in SHAPES:
        values = K.inputs(R, T, m, seed=31 * m + T)
        vbar, Fbar = adjoint_seeds(values, True)
        exact = arrays(R, T, m, *packs(values, True, vbar, Fbar, dtype=np.longdouble))
        plain = arrays(R, T, m, *packs(values, True, vbar, Fbar))
        c = arrays(R, T, m, *c_packs(values, True, vbar, Fbar))
        for name, want in exact.items():
            top = float(np.abs(want).max())
            worst_plain = max(worst_plain, float(np.abs(plain[name] - want).max()) / top)
            worst_c = max(worst_c, float(np.abs(c[name] - want).max()) / top)
    print(f"numpy evaluation {worst_plain:.3g}, C restatement {worst_c:.3g}, bound {4 * worst_plain:.3g}")
    assert worst_plain > 0.0
    assert worst_c <= 4.0 * worst_plain, (worst_c, worst_plain)


def test_the_probe_shapes_cover_what_the_contract_names():
    """every m meets every R class with and without a mask; T = 1, 2, 3 and 33 all occur; no case passes R T m m = 8 000 doubles"""
    for W in (1, 2, 4):
        shapes = K.kalman_shapes(W)
        assert {T for _, T, _, _ in shapes} == set(K.KAL_T)
        assert max(R * T * m * m for R, T, m, _ in shapes) <= K.CAP
        for m in K.KAL_M:
            S_ = 64 * W // K.group_lanes(m)
            for R in {1, 2, S_ - 1, S_, S_ + 1, 2 * S_ + 1} - {0}:
                assert {masked for R_, _, m_, masked in shapes if (R_, m_) == (R, m)} == {False, True}, (W, m, R)


# --------------------------------------------------------------------------- 5. source
def test_the_source_does_not_grow_with_t():
    """T = 50 / 200 / 500: the density function is less than 2 % apart (the digits of constants), and so is the whole source where it has
    the same parts: at T = 500 the packed filter result (13 000 doubles) does not fit the LDS of the generated expand function, which
    then runs on the host as for every long stage (the density keeps it in device memory)."""
    src, mid, long = (kalman_models.example(T=T, seasonal_period=12).compile()._source for T in (50, 200, 500))
    print(f"T = 50: {len(src)}, T = 200: {len(mid)}, T = 500: {len(long)} characters")
    assert "nphip_expand(" in src and "nphip_expand(" in mid
    assert abs(len(mid) - len(src)) < 0.02 * len(src), (len(src), len(mid))
    density = [len(v.split("nphip_expand(")[0]) for v in (src, mid, long)]
    assert max(density) - min(density) < 0.02 * min(density), density


def test_the_source_calls_the_kalman_routines_once_each():
    src = kalman_models.example(T=50, seasonal_period=12).compile()._source
    assert src.count('#include "chain_kalman.h"') >= 1
    density, expand = src.split("nphip_expand(", 1)
    assert density.count("nphip_kalman::forward<1, 50, 4, true>(") == 1 and density.count("nphip_kalman::backward<1, 50, 4, true>(") == 1
    assert density.count("nphip_kalman::") == 2
    assert expand.count("nphip_kalman::forward<1, 50, 4, true>(") == 1 and "nphip_kalman::backward" not in expand      # filtered_level: generated device code
    panel = kalman_models.example(**kalman_models.PANEL).compile()._source
    assert "nphip_kalman::forward<5, 20, 2, true>(" in panel and "nphip_kalman::backward<5, 20, 2, true>(" in panel
    ar = kalman_models.ar(**kalman_models.AR).compile()._source
    assert "nphip_kalman::forward<1, 64, 3, false>(" in ar and "nphip_kalman::backward<1, 64, 3, false>(" in ar and "(const double*)nullptr" in ar


def test_a_model_without_the_stage_does_not_see_the_header():
    from nutpie_amd.timeseries import garch11_model, regime_switching_model

    for model in (garch11_model(), regime_switching_model(T=20)):
        src = model.compile()._source
        assert "chain_kalman" not in src and "nphip_kalman" not in src


def test_waves_stay_free_and_the_limit_on_the_state():
    from nutpie_amd.density import compile_density, data_layout

    mod = kalman_models.example(**kalman_models.EXAMPLE)
    assert mod.compile()._waves == 1           # (chosen from the LDS the model needs, not forced)
    c = mod.compile(waves_per_chain=2)
    assert c._waves == 2
    assert os.path.exists(compile_density(c._source, data_layout(c._data), c.n_dim, waves=2))      # cross-compiles for gfx950
    with pytest.raises(ValueError, match="8"):
        ir_kalman(1, 3, 9, free=True)[0].compile()
    assert ir_kalman(1, 3, 8, free=True)[0].compile()._source.count("nphip_kalman::forward<1, 3, 8, false>") == 1


def test_a_kalman_stage_and_a_cholesky_compile_together_at_one_wave():
    from nutpie_amd.density import compile_density, data_layout

    c = kalman_models.kalman_with_cholesky().compile()
    assert c._waves == 1 and '#include "chain_linalg.h"' in c._source and '#include "chain_kalman.h"' in c._source
    assert os.path.exists(compile_density(c._source, data_layout(c._data), c.n_dim, waves=1))
    with pytest.raises(ValueError):
        kalman_models.kalman_with_cholesky().compile(waves_per_chain=2)


def test_malformed_arguments_are_value_errors():
    mod = S.Model()
    mod.dim("series", 3)
    mod.dim("time", 10)
    mod.dim("state", 2)
    steps = mod.product("series", "time")
    kk = mod.product("state", "state")
    y = mod.param("y", dim=steps.name)
    good = dict(design=mod.param("z", dim="state"), obs_var=1.0, transition=mod.param("Tm", dim=kk.name), state_cov=mod.param("Q", dim=kk.name),
                init_mean=0.0, init_cov=mod.param("P0", dim=kk.name))
    with pytest.raises(ValueError, match="outer"):
        S.kalman_marginal_lpdf(y, along="series", **good)
    with pytest.raises(ValueError, match="names no axis"):
        S.kalman_marginal_lpdf(y, along="days", **good)
    with pytest.raises(ValueError, match="transition"):
        S.kalman_marginal_lpdf(y, along="time", **{**good, "transition": mod.param("q", dim="time")})
    with pytest.raises(ValueError, match="init_mean"):
        S.kalman_marginal_lpdf(y, along="time", **{**good, "init_mean": mod.param("a3", dim="series")})
    with pytest.raises(ValueError, match="obs_var"):
        S.kalman_marginal_lpdf(y, along="time", **{**good, "obs_var": mod.param("h2", dim="state")})
    with pytest.raises(ValueError, match="design"):
        S.kalman_marginal_lpdf(y, along="time", **{**good, "design": 1.0})
    with pytest.raises(ValueError, match="observed"):
        S.kalman_marginal_lpdf(y, along="time", observed=mod.param("o", dim=steps.name), **good)
    with pytest.raises(ValueError, match="fixed-size"):
        S.kalman_marginal_lpdf(1.0, **good)
    assert S._topo([S.kalman_marginal_lpdf(y, along="time", **good)])[-1].op == "sum"
    stage = lambda e: next(n for n in S._topo([e]) if n.op == "kalman_fwd")      # noqa: E731
    assert stage(S.kalman_marginal_lpdf(y, along="time", **good)).payload == (3, 10, 2, False)
    assert stage(S.kalman_marginal_lpdf(y, **good)).payload == (1, 30, 2, False)      # without along: the rows are one series
    # the filtered state with the density's arguments is the density's stage
    assert stage(S.kalman_filtered_state(y, along="time", **good)) is stage(S.kalman_marginal_lpdf(y, along="time", **good))


# --------------------------------------------------------------------------- 6. tracer
def test_the_torch_op_traces_into_one_stage_and_agrees_with_the_symbolic_example():
    from nutpie_amd.torch_trace import trace

    for shape in (kalman_models.EXAMPLE, kalman_models.PANEL):
        sym = kalman_models.example(**shape).compile()
        D, logp = kalman_models.op_twin(**shape)
        assert D == sym.n_dim
        tr = trace(logp, D)
        nodes = S._topo([tr.model.logp_expr()])
        assert sum(n.op == "kalman_fwd" for n in nodes) == 1 and not any(n.op == "kalman_bwd" for n in nodes)
        traced = tr.compile()
        assert traced._source.count("nphip_kalman::forward<") == 1 and traced._source.count("nphip_kalman::backward<") == 1
        x = kalman_models.points(kalman_models.example(**shape), 16, seed=2)
        lp_s, g_s = sym.logp_and_grad_numpy(x)
        lp_t, g_t = traced.logp_and_grad_numpy(x)
        assert np.abs(lp_t - lp_s).max() <= 1e-12 * np.abs(lp_s).max()
        assert np.abs(g_t - g_s).max() <= 1e-12 * np.abs(g_s).max()


def test_the_eager_op_passes_gradcheck_and_equals_the_plain_loop():
    import torch

    from nutpie_amd.torch_trace import kalman_marginal

    values = K.inputs(2, 6, 3, seed=8)
    y, Z, h, Tm, Q, a0, P0 = (torch.tensor(values[k], requires_grad=True) for k in (0, 2, 3, 4, 5, 6, 7))
    obs = torch.tensor(values[1])
    obs[0, 2] = 0.0
    assert torch.autograd.gradcheck(lambda *a: kalman_marginal(*a, observed=obs), (y, Z, h, Tm, Q, a0, P0))
    assert torch.autograd.gradcheck(kalman_marginal, (y, Z[0, 0], h[0, 0], Tm, Q, a0, P0))      # a design row and a variance for all steps
    value, *_ = torch_reference(values[:1] + (obs.numpy(),) + values[2:], True)
    assert abs(float(kalman_marginal(y, Z, h, Tm, Q, a0, P0, observed=obs).sum().detach()) - value) <= 1e-12 * abs(value)
    with pytest.raises(ValueError):
        kalman_marginal(y, Z, h, Tm[:2], Q, a0, P0)
    with pytest.raises(ValueError):
        kalman_marginal(y, Z[:, :3], h, Tm, Q, a0, P0)


def test_a_transition_per_series_is_not_compiled():
    import torch

    from nutpie_amd.torch_trace import UnsupportedTorchOp, kalman_marginal, trace

    y = torch.randn(4, 5, dtype=torch.float64)
    eye = torch.eye(2, dtype=torch.float64)

    def logp(x):
        Tm = torch.tanh(x[:, :16]).reshape(-1, 4, 2, 2)
        return kalman_marginal(y[None] + x[:, 16:17, None], torch.ones(2, dtype=torch.float64), 1.0, Tm, eye, 0.0, eye).sum(-1)

    with pytest.raises(UnsupportedTorchOp):
        trace(logp, 17)


# --------------------------------------------------------------------------- 7. the examples
def test_the_examples_equal_their_twins_and_report_the_filtered_level():
    import torch

    for shape in (kalman_models.EXAMPLE, kalman_models.PANEL, dict(T=30)):
        mod = kalman_models.example(**shape)
        c = mod.compile()
        D, logp = kalman_models.twin(**shape)
        assert D == c.n_dim == (4 if shape.get("seasonal_period") else 3)
        x = kalman_models.points(mod, 6, seed=3)
        xt = torch.tensor(x, requires_grad=True)
        value = logp(xt)
        value.sum().backward()
        lp, g = c.logp_and_grad_numpy(x)
        assert np.abs(lp - value.detach().numpy()).max() <= 1e-12 * np.abs(lp).max()
        assert np.abs(g - xt.grad.numpy()).max() <= 1e-12 * np.abs(g).max()
        level = np.asarray(c._expand_func(x, **c._data)["filtered_level"])
        R, T = shape.get("R", 1), shape["T"]
        assert level.shape == ((6, R, T) if R > 1 else (6, T)) and np.isfinite(level).all()
        assert (mod._data["observed"] == 0).any() and (mod._data["observed"] == 1).any()
    mod = kalman_models.ar(**kalman_models.AR)
    D, logp = kalman_models.ar_twin(**kalman_models.AR)
    x = kalman_models.points(mod, 6, seed=4)
    xt = torch.tensor(x, requires_grad=True)
    value = logp(xt)
    value.sum().backward()
    lp, g = mod.compile().logp_and_grad_numpy(x)
    assert np.abs(lp - value.detach().numpy()).max() <= 1e-12 * np.abs(lp).max()
    assert np.abs(g - xt.grad.numpy()).max() <= 1e-12 * np.abs(g).max()
    assert np.abs(g[:, :3]).min() > 0.0          # the coefficients of the transition matrix: reached through Tbar
