"""Per-chain dense matrices in the compiled densities (symbolic cholesky / solve_lower, traced MultivariateNormal with a covariance
that depends on parameters): numpy evaluation, gradients, the generated source; no GPU."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import matrix_models as mm  # noqa: E402

from nutpie_amd import symbolic as S  # noqa: E402


def _central_diff(f, x, h=1e-6):
    g = np.zeros_like(x)
    for i in range(x.size):
        e = np.zeros_like(x)
        e[i] = h
        g[i] = (f(x + e) - f(x - e)) / (2 * h)
    return g


def test_matrix_stages_evaluate_as_numpy_linalg():
    rng = np.random.default_rng(0)
    K, N = 4, 3
    m = S.Model()
    m.dim("k", K)
    m.dim("n", N)
    kk, kn = m.product("k", "k"), m.product("k", "n")
    a = m.param("a", dims=("k", "k"))
    b = m.param("b", dims=("k", "n"))
    A = m.data("shift", (K * np.eye(K)).reshape(-1), dim=kk.name) + a * 0.3
    L = S.cholesky(A)
    X = S.solve_lower(L, b)
    x = rng.normal(size=(5, m.n_dim))
    Lv, Xv = S.evaluate([L, X], x, m._data)
    for r in range(5):
        Am = K * np.eye(K) + 0.3 * x[r, :K * K].reshape(K, K)
        Am = np.tril(Am) + np.tril(Am, -1).T                 # (the lower triangle is what is read)
        Lr = np.linalg.cholesky(Am)
        np.testing.assert_allclose(Lv[r].reshape(K, K), Lr, rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(Xv[r].reshape(K, N), np.linalg.solve(Lr, x[r, K * K:].reshape(K, N)), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("K", [1, 2, 3, 8, 32])
@pytest.mark.parametrize("N", [1, 85])
def test_gp_gradient_matches_central_differences(K, N):
    m = mm.gp_rows(K, N)
    c = m.compile()
    rng = np.random.default_rng(K * 100 + N)
    for _ in range(2):
        x = np.concatenate([[-0.2, -0.4, -1.5], 0.3 * rng.normal(size=K)]) + 0.05 * rng.normal(size=3 + K)
        lp, g = c.logp_and_grad_numpy(x[None])
        want = _central_diff(lambda z: c.logp_and_grad_numpy(z[None])[0][0], x)
        assert np.isfinite(lp[0])
        np.testing.assert_allclose(g[0], want, rtol=1e-5, atol=1e-5 * max(1.0, abs(lp[0])))


def test_gp_logp_matches_scipy():
    from scipy.stats import multivariate_normal

    K, N = 8, 85
    m = mm.gp_rows(K, N)
    c = m.compile()
    x = np.concatenate([[-0.2, -0.4, -1.5], np.linspace(-0.3, 0.3, K)])
    lp, _ = c.logp_and_grad_numpy(x[None])
    t = np.linspace(0.0, 3.0, K)
    cov = math.exp(-0.4) * np.exp(-0.5 * (t[:, None] - t[None, :]) ** 2 * math.exp(0.8)) + math.exp(-3.0) * np.eye(K)
    y = m._data["y"].reshape(K, N)
    want = multivariate_normal(x[3:], cov).logpdf(y.T).sum()
    want += sum(-0.5 * (v + 0.5) ** 2 - 0.5 * math.log(2 * math.pi) for v in x[:3]) + sum(-0.5 * v**2 - 0.5 * math.log(2 * math.pi) for v in x[3:])
    np.testing.assert_allclose(lp[0], want, rtol=1e-12)


def test_not_positive_definite_is_a_nonfinite_density():
    m = S.Model()
    m.dim("k", 2)
    kk = m.product("k", "k")
    r = m.param("r")
    A = m.data("one", np.array([1.0, 0.0, 0.0, 1.0]), dim=kk.name) + r * m.data("off", np.array([0.0, 1.0, 1.0, 0.0]), dim=kk.name)
    m.add_logp(S.log_det_chol(S.cholesky(A)))
    c = m.compile()
    lp, g = c.logp_and_grad_numpy(np.array([[0.5], [2.0]]))
    assert np.isfinite(lp[0]) and not np.isfinite(lp[1])
    np.testing.assert_allclose(lp[0], 0.5 * math.log(1 - 0.25), rtol=1e-13)


@pytest.mark.parametrize("fill", ["lower", "asymmetric", "symmetric"])
def test_cholesky_gradient_is_that_of_the_lower_triangle_it_reads(fill):
    # only the lower triangle of A is read: its gradient is exact whatever the upper triangle holds
    m = S.Model()
    m.dim("k", 3)
    kk = m.product("k", "k")
    a, b, c_, d = m.param("a"), m.param("b"), m.param("c"), m.param("d")
    e = S.exp
    lower = {(0, 0): e(a), (1, 0): b, (1, 1): e(c_), (2, 0): 0.3 * b, (2, 1): d, (2, 2): e(a) + 1.0}
    upper = {"lower": lambda i, j: 0.0, "asymmetric": lambda i, j: 2.0 * d + 1.0, "symmetric": lambda i, j: lower[(j, i)]}[fill]
    A = S.stack([lower[(i, j)] if j <= i else upper(i, j) for i in range(3) for j in range(3)], kk)
    L = S.cholesky(A)
    m.add_logp(S.log_det_chol(L) + S.elem(L, 3) + S.elem(L, 7) * S.elem(L, 6))
    cm = m.compile()
    rng = np.random.default_rng(3)
    for _ in range(3):
        x = np.array([0.8, 0.1, 0.5, -0.2]) + 0.1 * rng.normal(size=4)
        lp, g = cm.logp_and_grad_numpy(x[None])
        want = _central_diff(lambda z: cm.logp_and_grad_numpy(z[None])[0][0], x)
        np.testing.assert_allclose(g[0], want, rtol=1e-6, atol=1e-7)


def test_lkj_corr_cholesky_normalises_for_k2():
    # K = 2: L = [[1, 0], [r, sqrt(1 - r^2)]] and the density of r integrates to one
    from scipy.integrate import quad

    for eta in (1.0, 2.0, 3.5):
        m = S.Model()
        m.dim("k", 2)
        kk = m.product("k", "k")
        r = m.param("r", lower=-1.0, upper=1.0)
        L = S.stack([1.0, 0.0, r, S.sqrt(1.0 - r * r)], kk)
        lp = S.lkj_corr_cholesky_lpdf(L, eta)

        def dens(v):
            raw = math.log((v + 1) / (1 - v))
            return math.exp(S.evaluate([lp], np.array([[raw]]), m._data)[0][0])

        assert abs(quad(dens, -1, 1)[0] - 1.0) < 1e-8


@pytest.mark.parametrize("eta", [1.0, 2.0, 3.0])
def test_lkj_normalising_constant_for_k3_by_quadrature(eta):
    # the integral of det(R)^(eta - 1) over 3 x 3 correlation matrices, (r12, r13, r23) with det(R) > 0, is exp(-log_norm)
    from scipy.integrate import tplquad

    def det(r23, r13, r12):
        return max(1.0 - r12 * r12 - r13 * r13 - r23 * r23 + 2.0 * r12 * r13 * r23, 0.0) ** (eta - 1.0)

    def bound(sign):
        return lambda r12, r13: r12 * r13 + sign * math.sqrt(max((1 - r12 * r12) * (1 - r13 * r13), 0.0))

    val, _ = tplquad(det, -1, 1, -1, 1, bound(-1), bound(1), epsabs=1e-11, epsrel=1e-10)
    np.testing.assert_allclose(-math.log(val), S._lkj_log_norm(eta, 3), rtol=1e-8)


def test_lkj_cholesky_cov_matches_the_pymc_formula():
    K, eta = 3, 2.0
    m, L = mm.lkj_prior(K, eta)
    rng = np.random.default_rng(4)
    x = 0.4 * rng.normal(size=(3, m.n_dim))
    lp = S.evaluate([m.logp_expr()], x, m._data)[0]
    from scipy.special import gammaln

    for r in range(3):
        packed = x[r].copy()
        diag = [i * (i + 1) // 2 + i for i in range(K)]
        Lm = np.zeros((K, K))
        Lm[np.tril_indices(K)] = packed
        Lm[np.diag_indices(K)] = np.exp(Lm[np.diag_indices(K)])
        sd = np.sqrt((Lm**2).sum(1))
        corr_chol = Lm / sd[:, None]
        # LKJ on the correlation's factor + HalfNormal(1) sds + Jacobians (sd scaling, log diagonal)
        c = 0.0
        for i in range(1, K):
            b = eta + (K - i - 1) / 2.0
            c += (2 * eta - 2 + K - i) * (K - i) * math.log(2) + (K - i) * (2 * gammaln(b) - gammaln(2 * b))
        want = -c + sum((K - i - 1 + 2 * eta - 2) * math.log(corr_chol[i, i]) for i in range(1, K))
        want += sum(math.log(2 / math.pi) / 2 - 0.5 * s**2 for s in sd)
        want += sum(math.log(corr_chol[i, i]) - i * math.log(sd[i]) for i in range(K)) + packed[diag].sum()
        np.testing.assert_allclose(lp[r], want, rtol=1e-12)
        np.testing.assert_allclose(S.evaluate([L], x[r:r + 1], m._data)[0][0].reshape(K, K), Lm, rtol=1e-14)


def test_the_source_calls_the_device_routines_and_keeps_one_wave():
    c = mm.gp_rows(3, 5).compile()
    src = c._source
    assert '#include "chain_linalg.h"' in src
    for fn in ("cholesky<3>", "solve_lower<3, 5>", "solve_lower_t<3, 5, 5, 1>", "solve_lower_adj_l<3, 5>", "cholesky_adj<3>"):
        assert f"nphip_la::{fn}(" in src, fn
    assert c._waves == 1
    with pytest.raises(ValueError, match="waves_per_chain=1"):
        mm.gp_rows(3, 5).compile(waves_per_chain=2)
    with pytest.raises(ValueError, match="up to 32 x 32"):
        mm.gp_rows(33, 2).compile()


def test_models_without_matrices_generate_the_same_source():
    # the traced model with a CONSTANT scale_tril keeps its product with the inverse: the source is the one from before the matrix stages
    import hashlib

    import torch_models as TM

    from nutpie_amd.torch_trace import trace

    D, fn, batched, shared = TM.negbin_and_pairwise()
    src = trace(fn, D, batched=batched, shared_data=shared).compile()._source
    assert "chain_linalg" not in src and "nphip_la::" not in src
    assert hashlib.sha256(src.encode()).hexdigest() == "7d10ae563eafedc05c12df3a2042207a663dfe443e94e97b1966ec01178d5c85"


def test_generated_density_compiles_for_gfx950():
    from nutpie_amd.density import compile_density, data_layout

    c = mm.gp_rows(8, 85).compile()
    path = compile_density(c._source, data_layout(c._data), c.n_dim)
    assert os.path.exists(path)


# ---------------------------------------------------------------------------------------------------------- the torch front end
def _corr_from(z, K):
    import torch

    rows, at = [], 0
    for i in range(K):
        parts = []
        for j in range(K):
            if j < i:
                parts.append(z[at])
                at += 1
            else:
                parts.append(torch.ones((), dtype=torch.float64) if j == i else torch.zeros((), dtype=torch.float64))
        r_ = torch.stack(parts)
        rows.append(r_ / torch.sqrt((r_ * r_).sum()))
    W = torch.stack(rows)
    return W @ W.T


def _mvn_density(K, N, form):
    import torch
    from torch.distributions import MultivariateNormal

    y = torch.as_tensor(np.random.default_rng(5).normal(size=(N, K)))

    def logp(x):
        s = x[0, :K].exp()
        mu = x[0, K:2 * K]
        C = s[:, None] * _corr_from(x[0, 2 * K:], K) * s[None, :]
        if form == "cov":
            d = MultivariateNormal(mu, covariance_matrix=C)
        elif form == "scale_tril":
            d = MultivariateNormal(mu, scale_tril=torch.linalg.cholesky(C))
        else:   # a right-side solve with the upper factor: z^T = (y - mu)^T U^-1, U = L^T
            U = torch.linalg.cholesky(C, upper=True)
            z = torch.linalg.solve_triangular(U, (y - mu), upper=True, left=False)
            return (-0.5 * (z * z).sum() - N * torch.log(torch.diagonal(U)).sum()).reshape(1)
        return d.log_prob(y).sum().reshape(1)

    return logp, 2 * K + K * (K - 1) // 2


@pytest.mark.parametrize("form", ["cov", "scale_tril", "right_upper"])
@pytest.mark.parametrize("K,N", [(2, 7), (3, 85), (5, 1)])
def test_traced_mvnormal_with_a_parameter_covariance_matches_autograd(form, K, N):
    import torch

    from nutpie_amd.torch_trace import trace

    logp, nd = _mvn_density(K, N, form)
    c = trace(logp, nd).compile()
    rng = np.random.default_rng(K + N)
    for _ in range(3):
        x = 0.5 * rng.normal(size=(1, nd))
        lp, g = c.logp_and_grad_numpy(x)
        xt = torch.tensor(x, requires_grad=True)
        out = logp(xt)
        out.backward()
        np.testing.assert_allclose(lp[0], out.item(), rtol=1e-10)
        np.testing.assert_allclose(g[0], xt.grad.numpy()[0], rtol=1e-10, atol=1e-10 * abs(out.item()))


def test_traced_mvnormal_compiles_with_auto():
    import nutpie_amd

    logp, nd = _mvn_density(3, 10, "cov")
    model = nutpie_amd.from_torch_density(nd, logp, compile="auto")
    assert "nphip_la::cholesky<3>" in model._source


def test_a_traced_matrix_past_the_limit_falls_back_to_the_eager_form():
    import torch

    import nutpie_amd
    from nutpie_amd.torch_trace import UnsupportedTorchOp, trace

    n = 40
    d2 = torch.as_tensor((np.linspace(0, 4, n)[:, None] - np.linspace(0, 4, n)[None, :]) ** 2)
    y = torch.as_tensor(np.random.default_rng(1).normal(size=n))

    def logp(x):
        C = torch.exp(2 * x[:, 0, None, None]) * torch.exp(-0.5 * d2) + torch.exp(2 * x[:, 1, None, None]) * torch.eye(n, dtype=torch.float64)
        return torch.distributions.MultivariateNormal(torch.zeros(n, dtype=torch.float64), covariance_matrix=C).log_prob(y)

    with pytest.raises(UnsupportedTorchOp, match="up to 32 x 32"):
        trace(logp, 2)
    with pytest.warns(UserWarning, match="up to 32 x 32"):
        model = nutpie_amd.from_torch_density(2, logp, compile="auto")
    assert not hasattr(model, "_source")


def test_correlated_radon_example_matches_its_torch_density():
    import torch

    from nutpie_amd.radon import correlated_radon_model, correlated_radon_torch_density

    c = correlated_radon_model().compile()
    D, logp = correlated_radon_torch_density()
    assert c.n_dim == D and c._waves == 1
    x = 0.3 * np.random.default_rng(6).normal(size=(4, D))
    lp, g = c.logp_and_grad_numpy(x)
    xt = torch.tensor(x, requires_grad=True)
    out = logp(xt)
    out.sum().backward()
    np.testing.assert_allclose(lp, out.detach().numpy(), rtol=1e-12)
    np.testing.assert_allclose(g, xt.grad.numpy(), rtol=1e-10, atol=1e-10)


def test_a_deterministic_on_a_matrix_stage_is_generated_device_code():
    from nutpie_amd.density import compile_density, data_layout

    c = mm.gp_rows(4, 6, factor_deterministic=True).compile()
    expand_src = c._source[c._source.index("nphip_expand("):]
    assert "nphip_la::cholesky<4>(" in expand_src
    x = np.concatenate([[-0.2, -0.4, -1.5], np.zeros(4)])[None]
    got = c._expand_func(x, **c._data)["cov_chol"]
    t = np.linspace(0.0, 3.0, 4)
    cov = math.exp(-0.4) * np.exp(-0.5 * (t[:, None] - t[None, :]) ** 2 * math.exp(0.8)) + math.exp(-3.0) * np.eye(4)
    np.testing.assert_allclose(np.asarray(got).reshape(4, 4), np.linalg.cholesky(cov), rtol=1e-13)
    assert os.path.exists(compile_density(c._source, data_layout(c._data), c.n_dim))
