"""Hidden Markov models in the symbolic IR (nutpie_amd/symbolic.py: hmm_marginal_lpdf, hmm_state_prob, Model.transition_matrix), the
torch front end (nutpie_amd/torch_trace.py: hmm_marginal) and the plain-C restatement of the device routines' order contract
(tests/fixtures/hmm_reference.c) — everything that needs no GPU.  DESIGN.md §11.8."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import hmm_models  # noqa: E402
import hmm_reference as H  # noqa: E402

from nutpie_amd import symbolic as S  # noqa: E402


# --------------------------------------------------------------------------- helpers
def ir_hmm(R, T, K, free=False, logE=None, P=None, pi=None):
    """a Model whose density is hmm_marginal_lpdf of R series; the three operands are data, or (``free``) unconstrained parameters
    ``[logE (R T K), P (K K), pi (K)]``.  Returns (model, logE expr, P expr, pi expr, along)."""
    m = S.Model()
    m.dim("state", K)
    m.dim("time", T)
    if R == 1:
        steps, along = "time", None
    else:
        m.dim("series", R)
        steps, along = m.product("series", "time").name, "time"
    d = m.product(steps, "state")
    kk = m.product("state", "state")
    if free:
        le, Pm, p0 = m.param("logE", dim=d.name), m.param("P", dim=kk.name), m.param("pi", dim="state")
    else:
        le, Pm, p0 = m.data("logE", np.reshape(logE, -1), dim=d.name), m.data("P", np.reshape(P, -1), dim=kk.name), m.data("pi", pi, dim="state")
        m.param("unused")
    m.add_logp(S.hmm_marginal_lpdf(le, Pm, p0, along=along))
    return m, le, Pm, p0, along


def inputs(R, T, K, seed, scale=3.0, shift=0.0, impossible=False):
    rng = np.random.default_rng(seed)
    logE = scale * rng.normal(size=(R, T, K)) + shift
    if impossible and K > 1:
        logE[:, :, K - 1] = -np.inf
    return logE, rng.uniform(0.1, 1.0, size=(K, K)), rng.uniform(0.1, 1.0, size=K)


def mp_enumerate(logE, P, pi):
    """log of the sum over all K^T state paths, 50 digits"""
    import mpmath as mp

    mp.mp.dps = 50
    R, T, K = logE.shape
    e = [[[mp.exp(mp.mpf(float(v))) if np.isfinite(v) else mp.mpf(0) for v in row] for row in series] for series in logE]
    Pm = [[mp.mpf(float(v)) for v in row] for row in P]
    total = mp.mpf(0)
    for r in range(R):
        s = mp.mpf(0)
        for path in itertools.product(range(K), repeat=T):
            w = mp.mpf(float(pi[path[0]])) * e[r][0][path[0]]
            for t in range(1, T):
                w *= Pm[path[t - 1]][path[t]] * e[r][t][path[t]]
            s += w
        total += mp.log(s)
    return total


def mp_forward(logE, P, pi):
    """the same value by the unscaled forward recursion at 50 digits (no rounding that matters, no K^T paths)"""
    import mpmath as mp

    mp.mp.dps = 50
    R, T, K = logE.shape
    Pm = mp.matrix([[mp.mpf(float(v)) for v in row] for row in P])
    total = mp.mpf(0)
    for r in range(R):
        a = mp.matrix([[mp.mpf(float(pi[k])) * mp.exp(mp.mpf(float(logE[r, 0, k]))) for k in range(K)]])
        for t in range(1, T):
            a = a * Pm
            a = mp.matrix([[a[0, k] * mp.exp(mp.mpf(float(logE[r, t, k]))) for k in range(K)]])
        total += mp.log(sum(a[0, k] for k in range(K)))
    return total


def logaddexp_recursion(logE, P, pi):
    """a plain float64 forward recursion in the log domain (numpy logaddexp, states in ascending order)"""
    R, T, K = logE.shape
    with np.errstate(all="ignore"):
        logP = np.log(P)
        total = 0.0
        for r in range(R):
            la = np.log(pi) + logE[r, 0]
            for t in range(1, T):
                la = np.array([np.logaddexp.reduce(la + logP[:, j]) for j in range(K)]) + logE[r, t]
            total += np.logaddexp.reduce(la)
    return total


SMALL = [(R, T, K) for K in (1, 2, 3) for T in (1, 2, 5) for R in (1, 3)]


# --------------------------------------------------------------------------- 1. value
@pytest.mark.parametrize("R,T,K", SMALL)
def test_value_is_the_sum_over_all_state_paths(R, T, K):
    """P with rows that do not sum to one, pi that does not either, and (K > 1; with one state the value would be -inf) the last
    state impossible at every step: the IR's numpy evaluation against the enumeration of the K^T paths at 50 digits."""
    logE, P, pi = inputs(R, T, K, seed=R + 10 * T + 100 * K, impossible=True)
    m, *_ = ir_hmm(R, T, K, logE=logE, P=P, pi=pi)
    got = S.evaluate([m.logp_expr()], np.zeros((1, 1)), m._data)[0][0]
    want = float(mp_enumerate(logE, P, pi))
    assert abs(got - want) <= 1e-13 * abs(want), (got, want)


# --------------------------------------------------------------------------- 2. gradient
def torch_reference(logE, P, pi):
    import torch

    le, Pm, p0 = (torch.tensor(v, requires_grad=True) for v in (logE, P, pi))
    la = torch.log(p0) + le[:, 0]
    for t in range(1, le.shape[1]):
        la = torch.logsumexp(la[:, :, None] + torch.log(Pm)[None], dim=1) + le[:, t]
    value = torch.logsumexp(la, dim=-1).sum()
    value.backward()
    g_P = Pm.grad.numpy() if Pm.grad is not None else np.zeros_like(P)      # (T = 1: P is not used)
    return float(value.detach()), le.grad.numpy(), g_P, p0.grad.numpy()


@pytest.mark.parametrize("K,T", [(2, 5), (3, 20), (4, 50), (8, 64), (16, 65), (3, 1)])
@pytest.mark.parametrize("R", [1, 3])
def test_gradient_equals_autograd_of_a_log_domain_recursion(R, K, T):
    """The IR gradient (numpy evaluation) with respect to logE, P and pi against torch.autograd of an independent recursion:
    1e-12 of the largest element of each gradient.  T = 1: the adjoint of P is zero."""
    logE, P, pi = inputs(R, T, K, seed=7 * K + T + R)
    m, *_ = ir_hmm(R, T, K, free=True)
    x = np.concatenate([logE.reshape(-1), P.reshape(-1), pi])[None]
    lp, g = m.compile().logp_and_grad_numpy(x)
    value, g_le, g_P, g_pi = torch_reference(logE, P, pi)
    assert abs(lp[0] - value) <= 1e-12 * abs(value)
    n = R * T * K
    for name, got, want in (("logE", g[0, :n], g_le.reshape(-1)), ("P", g[0, n:n + K * K], g_P.reshape(-1)), ("pi", g[0, n + K * K:], g_pi)):
        assert np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300), (name, np.abs(got - want).max(), np.abs(want).max())
    if T == 1:
        assert not g[0, n:n + K * K].any()


def test_second_derivatives_are_refused():
    m, le, Pm, p0, along = ir_hmm(1, 4, 2, free=True)
    prob = S.hmm_state_prob(le, Pm, p0, along=along)
    with pytest.raises(NotImplementedError):
        S.gradient(prob.sum(), m._params)


# --------------------------------------------------------------------------- 3. the C restatement
def test_c_restatement_against_mpmath():
    """The restatement of the device routines' order contract (scaled forward algorithm, tests/fixtures/hmm_reference.c) against the
    50-digit value, on the shapes of the enumeration test and on K = 16, T = 65 with logE = 30 N(0, 1) - 2000 (an unscaled recursion
    underflows there).  The bound is measured, not fixed: the largest relative error of a plain float64 log-domain recursion (numpy
    logaddexp) on the same inputs, times 4 — both are O(T K u) algorithms with different constants.  Measured: log-domain recursion
    4.18e-16, so the bound is 1.67e-15; the restatement's largest relative error is 3.13e-16."""
    cases = [inputs(R, T, K, seed=R + 10 * T + 100 * K, impossible=True) for R, T, K in SMALL]
    cases.append(inputs(1, 65, 16, seed=5, scale=30.0, shift=-2000.0))
    worst_plain = worst_c = 0.0
    for logE, P, pi in cases:
        R, T, K = logE.shape
        want = mp_forward(logE, P, pi)
        rel = lambda v: float(abs((v - want) / want))     # noqa: E731
        worst_plain = max(worst_plain, rel(logaddexp_recursion(logE, P, pi)))
        worst_c = max(worst_c, rel(H.value(logE, P, pi, R, T, K)))
    print(f"log-domain recursion {worst_plain:.3g}, C restatement {worst_c:.3g}, bound {4 * worst_plain:.3g}")
    assert worst_plain > 0.0
    assert worst_c <= 4.0 * worst_plain, (worst_c, worst_plain)


def test_c_restatement_equals_the_numpy_evaluation():
    """every packed array of both stages, not only the value"""
    R, T, K = 3, 7, 4
    logE, P, pi = inputs(R, T, K, seed=3)
    F = H.forward(logE, P, pi, R, T, K)
    B = H.backward(logE, P, F, R, T, K)
    row = lambda v: np.reshape(v, (1, -1))      # noqa: E731
    F_np = S._np_hmm("hmm_fwd", [row(logE), row(P), row(pi)], R, T, K, 1)[0]
    B_np = S._np_hmm("hmm_bwd", [row(logE), row(P), row(F_np)], R, T, K, 1)[0]
    np.testing.assert_allclose(F, F_np, rtol=1e-13)
    np.testing.assert_allclose(B, B_np, rtol=1e-13)


# --------------------------------------------------------------------------- 4. source
def test_the_source_does_not_grow_with_t():
    """T = 50 against T = 500: less than 2 %.  One call line per routine at either length, and the element-wise loops over the series'
    dimensions (``time``, ``time x state``) are written four iterations wide whatever T is — elsewhere a loop over a short
    dimension is written ceil(size / 64 W) wide, which would make T = 50 12 % shorter than T = 500.  Lengths differ only in the
    digits of constants: 0.1 %."""
    src = hmm_models.example(T=50, K=2).compile()._source
    long = hmm_models.example(T=500, K=2).compile()._source
    mid = hmm_models.example(T=200, K=2).compile()._source
    print(f"T = 50: {len(src)}, T = 200: {len(mid)}, T = 500: {len(long)} characters")
    assert abs(len(long) - len(mid)) < 0.02 * len(mid), (len(mid), len(long))
    assert abs(len(long) - len(src)) < 0.02 * len(src), (len(src), len(long))


def test_the_source_calls_the_hmm_routines():
    src = hmm_models.example(T=50, K=2).compile()._source
    assert src.count('#include "chain_hmm.h"') >= 1
    assert "nphip_hmm::forward<1, 50, 2>(" in src and "nphip_hmm::backward<1, 50, 2>(" in src and "nphip_hmm::transition_adjoint<1, 50, 2>(" in src
    assert "nphip_expand(" in src            # the smoothed probabilities: generated device code
    assert src.count("nphip_hmm::forward<") == 2     # once in the density, once in the expand function
    panel = hmm_models.example(**hmm_models.PANEL).compile()._source
    assert "nphip_hmm::forward<5, 20, 3>(" in panel and "nphip_hmm::backward<5, 20, 3>(" in panel


def test_a_model_without_an_hmm_does_not_see_the_header():
    from nutpie_amd.timeseries import garch11_model

    src = garch11_model().compile()._source
    assert "chain_hmm" not in src and "nphip_hmm" not in src


def test_waves_stay_free_and_the_limit_on_the_states():
    from nutpie_amd.density import compile_density, data_layout

    m = hmm_models.example(**hmm_models.EXAMPLE)
    assert m.compile()._waves == 1           # (chosen from the LDS the model needs, not forced)
    c = m.compile(waves_per_chain=2)
    assert c._waves == 2
    assert os.path.exists(compile_density(c._source, data_layout(c._data), c.n_dim, waves=2))
    big, *_ = ir_hmm(1, 3, 17, free=True)
    with pytest.raises(ValueError, match="16"):
        big.compile()
    assert ir_hmm(1, 3, 16, free=True)[0].compile()._source.count("nphip_hmm::forward<1, 3, 16>") == 1


def test_an_hmm_and_a_cholesky_compile_together_at_one_wave():
    from nutpie_amd.density import compile_density, data_layout

    c = hmm_models.hmm_with_cholesky().compile()
    assert c._waves == 1 and '#include "chain_linalg.h"' in c._source and '#include "chain_hmm.h"' in c._source
    assert os.path.exists(compile_density(c._source, data_layout(c._data), c.n_dim, waves=1))
    with pytest.raises(ValueError):
        hmm_models.hmm_with_cholesky().compile(waves_per_chain=2)


def test_malformed_arguments_are_value_errors():
    m = S.Model()
    m.dim("series", 3)
    m.dim("time", 10)
    m.dim("state", 2)
    steps = m.product("series", "time")
    le = m.param("le", dim=m.product(steps.name, "state").name)
    P = m.param("P", dim=m.product("state", "state").name)
    with pytest.raises(ValueError, match="outer"):
        S.hmm_marginal_lpdf(le, P, 0.5, along="series")
    with pytest.raises(ValueError, match="names no axis"):
        S.hmm_marginal_lpdf(le, P, 0.5, along="days")
    with pytest.raises(ValueError, match="transition"):
        S.hmm_marginal_lpdf(le, m.param("q", dim="time"), 0.5, along="time")
    with pytest.raises(ValueError, match="initial"):
        S.hmm_marginal_lpdf(le, P, m.param("p3", dim="series"), along="time")
    with pytest.raises(ValueError, match="product"):
        S.hmm_marginal_lpdf(m.param("flat", dim="time"), P, 0.5)
    assert S.hmm_marginal_lpdf(le, P, 0.5, along="time").args[0].args[0].payload == (3, 10, 2)
    assert S.hmm_marginal_lpdf(le, P, 0.5).args[0].args[0].payload == (1, 30, 2)      # without along: the rows are one series


# --------------------------------------------------------------------------- 5. tracer
def test_the_torch_op_traces_into_one_stage_and_agrees_with_the_symbolic_example():
    from nutpie_amd.torch_trace import trace

    for shape in (hmm_models.EXAMPLE, hmm_models.PANEL):
        sym = hmm_models.example(**shape).compile()
        D, logp = hmm_models.twin(**shape)
        assert D == sym.n_dim
        tr = trace(logp, D)
        nodes = S._topo([tr.model.logp_expr()])
        assert sum(n.op == "hmm_fwd" for n in nodes) == 1 and not any(n.op == "hmm_bwd" for n in nodes)
        traced = tr.compile()
        assert traced._source.count("nphip_hmm::forward<") == 1 and traced._source.count("nphip_hmm::backward<") == 1
        x = hmm_models.points(hmm_models.example(**shape), 16, seed=2)
        lp_s, g_s = sym.logp_and_grad_numpy(x)
        lp_t, g_t = traced.logp_and_grad_numpy(x)
        assert np.abs(lp_t - lp_s).max() <= 1e-12 * np.abs(lp_s).max()
        assert np.abs(g_t - g_s).max() <= 1e-12 * np.abs(g_s).max()


def test_the_eager_op_passes_gradcheck_and_equals_the_twin_formula():
    import torch

    from nutpie_amd.torch_trace import hmm_marginal

    rng = np.random.default_rng(8)
    le = torch.tensor(rng.normal(size=(2, 6, 3)), requires_grad=True)
    P = torch.tensor(rng.uniform(0.1, 1.0, size=(3, 3)), requires_grad=True)
    pi = torch.tensor(rng.uniform(0.1, 1.0, size=3), requires_grad=True)
    assert torch.autograd.gradcheck(hmm_marginal, (le, P, pi))
    value, *_ = torch_reference(le.detach().numpy(), P.detach().numpy(), pi.detach().numpy())
    assert abs(float(hmm_marginal(le, P, pi).sum()) - value) <= 1e-12 * abs(value)
    with pytest.raises(ValueError):
        hmm_marginal(le, P[:2], pi)


def test_a_matrix_per_series_is_not_compiled():
    import torch

    from nutpie_amd.torch_trace import UnsupportedTorchOp, hmm_marginal, trace

    le = torch.randn(4, 5, 2, dtype=torch.float64)

    def logp(x):
        P = torch.sigmoid(x[:, :16]).reshape(-1, 4, 2, 2)
        return hmm_marginal(le[None] + x[:, 16:17, None, None], P, 0.5).sum(-1)

    with pytest.raises(UnsupportedTorchOp):
        trace(logp, 17)


# --------------------------------------------------------------------------- 6. identity
@pytest.mark.parametrize("R,T,K", [(1, 9, 3), (4, 6, 2)])
def test_equal_rows_make_it_a_mixture(R, T, K):
    """with every row of P equal to pi the states are independent draws: sum_t logsumexp_k(log pi_k + logE[t][k])"""
    logE, _, pi = inputs(R, T, K, seed=11)
    pi = pi / pi.sum()
    m, *_ = ir_hmm(R, T, K, logE=logE, P=np.tile(pi, (K, 1)), pi=pi)
    got = S.evaluate([m.logp_expr()], np.zeros((1, 1)), m._data)[0][0]
    want = np.logaddexp.reduce(np.log(pi) + logE, axis=-1).sum()
    assert abs(got - want) <= 1e-12 * abs(want)


# --------------------------------------------------------------------------- 7. deterministics and the helper
@pytest.mark.parametrize("R", [1, 3])
def test_state_probabilities(R):
    T, K = 12, 3
    logE, P, pi = inputs(R, T, K, seed=21)
    m, le, Pm, p0, along = ir_hmm(R, T, K, free=True)
    x = np.concatenate([logE.reshape(-1), P.reshape(-1), pi])[None]
    smoothed, filtered = S.hmm_state_prob(le, Pm, p0, along=along), S.hmm_state_prob(le, Pm, p0, along=along, smoothed=False)
    assert smoothed.dim is le.dim and filtered.dim is le.dim
    sm, fl = (v[0].reshape(R * T, K) for v in S.evaluate([smoothed, filtered], x, m._data))
    assert np.abs(sm.sum(-1) - 1.0).max() <= 1e-14 and np.abs(fl.sum(-1) - 1.0).max() <= 1e-14
    assert np.abs(sm[T - 1::T] - fl[T - 1::T]).max() <= 1e-15          # at a series' last step the two coincide
    _, g = m.compile().logp_and_grad_numpy(x)
    np.testing.assert_array_equal(g[0, :R * T * K], sm.reshape(-1))    # the smoothed probability IS the gradient with respect to logE


def test_transition_matrix_helper():
    m = S.Model()
    P = m.transition_matrix("A", 3, concentration=2.0)
    assert P.dim is m._dims["A_k_x_A_k"] and m.n_dim == 6
    assert [m._unconstrained[f"A_{i}"][0] for i in range(3)] == ["A_0_simplex__", "A_1_simplex__", "A_2_simplex__"]
    m.dim("time", 4)
    le = m.data("le", np.zeros(12), dim=m.product("time", "A_k").name)
    m.add_logp(S.hmm_marginal_lpdf(le, P, 1.0 / 3.0))
    c = m.compile()
    x = np.random.default_rng(1).normal(size=(5, 6))
    out = c._expand_func(x, **c._data)
    A = np.asarray(out["A"]).reshape(5, 3, 3)
    assert (A > 0).all() and np.abs(A.sum(-1) - 1.0).max() <= 1e-15
    for i in range(3):       # row i of the matrix is the i-th simplex parameter
        np.testing.assert_array_equal(A[:, i], np.asarray(out[f"A_{i}"]))
    # emissions that do not tell the states apart and a stochastic matrix: the likelihood is 1 whatever the rows are, so the density
    # is the rows' Dirichlet(2) prior + the simplex Jacobians
    lp, _ = c.logp_and_grad_numpy(x)
    no_hmm = S.Model()
    no_hmm.transition_matrix("A", 3, concentration=2.0)
    want, _ = no_hmm.compile().logp_and_grad_numpy(x)
    np.testing.assert_allclose(lp, want, rtol=1e-13)


def test_the_example_reports_its_smoothed_probabilities():
    m = hmm_models.example(**hmm_models.PANEL)
    c = m.compile()
    x = hmm_models.points(m, 4, seed=3)
    out = c._expand_func(x, **c._data)
    prob = np.asarray(out["state_prob"])
    assert prob.shape == (4, 5 * 20, 3) and np.abs(prob.sum(-1) - 1.0).max() <= 1e-14
    assert (np.diff(np.asarray(out["mu"]), axis=-1) > 0).all()           # ordered means: the labels cannot switch
