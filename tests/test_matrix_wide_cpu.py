"""Matrix stages past 32 x 32 (csrc/wide_chain_linalg.h, Model.compile(wide_matrices=True)) without a GPU: which routines
the generated source calls and the limits, the sources that must not change, a source that does not grow with K, the host evaluation
against torch.autograd, the traced form, cross-compilation for gfx950, and the GP example against its torch twin."""
import hashlib
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import matrix_models as mm  # noqa: E402

from nutpie_amd import symbolic as S  # noqa: E402

ROUTINES = ("cholesky<{k}>", "solve_lower<{k}, {n}>", "solve_lower_t<{k}, {n}, {n}, 1>", "solve_lower_adj_l<{k}, {n}>", "cholesky_adj<{k}>")


def test_calls_and_limits():
    c = mm.gp_rows(33, 2).compile(wide_matrices=True)
    src = c._source
    assert '#include "wide_chain_linalg.h"' in src and "chain_linalg.h\"" not in src.replace("wide_chain_linalg.h", "")
    for fn in ROUTINES:
        assert f"nphip_lw::{fn.format(k=33, n=2)}(" in src, fn
    assert "nphip_la::" not in src
    narrow = mm.gp_rows(3, 5).compile(wide_matrices=True)
    assert '#include "chain_linalg.h"' in narrow._source and "nphip_lw::" not in narrow._source and narrow._waves == 1
    for fn in ROUTINES:
        assert f"nphip_la::{fn.format(k=3, n=5)}(" in narrow._source, fn
    with pytest.raises(ValueError, match="128 x 128"):
        mm.gp_rows(129, 1).compile(wide_matrices=True)
    assert mm.gp_rows(64, 1).compile(wide_matrices=True, waves_per_chain=4)._waves == 4
    assert mm.gp_rows(64, 1).compile(wide_matrices=True, waves_per_chain=2)._waves == 2
    # without the switch: refused as before, the message now names the option
    with pytest.raises(ValueError, match=r"up to 32 x 32 .*wide_matrices=True"):
        mm.gp_rows(33, 2).compile()


def test_a_narrow_stage_beside_a_wide_one_keeps_the_model_at_one_wave():
    m = mm.gp_rows(40, 1)
    m.dim("s", 3)
    ss = m.product("s", "s")
    A = m.data("small", (np.eye(3) * 2.0 + 0.1).reshape(-1), dim=ss.name) * S.exp(m.param("log_scale"))
    m.add_logp(-S.log_det_chol(S.cholesky(A)))
    c = m.compile(wide_matrices=True)
    assert c._waves == 1 and "nphip_la::cholesky<3>(" in c._source and "nphip_lw::cholesky<40>(" in c._source
    assert c._source.index('#include "chain_linalg.h"') < c._source.index('#include "wide_chain_linalg.h"')
    with pytest.raises(ValueError, match="waves_per_chain=1"):
        m.compile(wide_matrices=True, waves_per_chain=2)


def test_sources_without_the_switch_are_unchanged():
    # (sha256 of the generated source on the parent commit)
    for (K, N), want in {(3, 5): "9b44a30e2c26e28a9535999bc2c1fb84a36c812639d0f8f38ff5dcaac4933d62",
                         (32, 2): "30695b8cde6a0d694f381b55479aadc9705e0536ee5398609e96e2662c903cd6"}.items():
        assert hashlib.sha256(mm.gp_rows(K, N).generate(1)[0].encode()).hexdigest() == want
        assert mm.gp_rows(K, N).compile(wide_matrices=True)._source == mm.gp_rows(K, N).compile()._source


def _longest_run_of_literal_stores(src: str) -> int:
    longest = run = 0
    for line in src.splitlines():
        run = run + 1 if re.fullmatch(r"\s*M\d+\[\d+\] = \(?-?0x[0-9a-fp.+-]+\)?;", line) else 0
        longest = max(longest, run)
    return longest


def test_the_source_does_not_grow_with_the_matrix():
    sources = {}
    for K in (96, 128):
        m = mm.gp_rows(K, 1)
        c = m.compile(wide_matrices=True, waves_per_chain=1)
        sources[K] = c._source
        gen = m.generate(1)[1]
        assert gen.unroll(m._dims["k"]) == 2 and gen.unroll(m._dims["k_x_k"]) == 4
        assert _longest_run_of_literal_stores(c._source) <= 64
        density = c._source[:c._source.index("nphip_expand(")]
        assert density.count("    if (lane == 0) {") == 1      # (the scalar gradient rows only: no vector assembled by one lane)
    a, b = (s.splitlines() for s in sources.values())
    assert len(a) == len(b)
    differing = [(x, y) for x, y in zip(a, b) if x != y]
    constant = r"-?0x[0-9a-f.]+p[+-]?\d+|\d+"      # a hexadecimal floating-point literal or an integer
    assert differing and all(re.sub(constant, "#", x) == re.sub(constant, "#", y) for x, y in differing)      # only constants differ
    # the narrow form's diagonal, for comparison: one scalar read per row
    assert mm.gp_rows(32, 1).compile()._source.count("= M") > 32 > sources[128].count("= M")


def _gp_rows_torch(K, N, seed=0):
    """tests/matrix_models.gp_rows restated in torch: x = [log_amp, log_ls, log_noise, mu (K)]"""
    import torch

    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 3.0, K)
    d2 = (t[:, None] - t[None, :]) ** 2
    cov = 0.8**2 * np.exp(-0.5 * d2 / 0.7**2) + 0.1**2 * np.eye(K)
    y = torch.as_tensor(np.linalg.cholesky(cov) @ rng.normal(size=(K, N)) + 0.3)
    d2 = torch.as_tensor(d2)

    def logp(x):
        la, ll, ln, mu = x[0], x[1], x[2], x[3:]
        C = torch.exp(2 * la) * torch.exp(-0.5 * d2 * torch.exp(-2 * ll)) + torch.exp(2 * ln) * torch.eye(K, dtype=torch.float64)
        L = torch.linalg.cholesky(C)
        z = torch.linalg.solve_triangular(L, y - mu[:, None], upper=False)
        lp = -0.5 * (z * z).sum() - N * torch.log(torch.diagonal(L)).sum() - N * K * 0.5 * np.log(2 * np.pi)
        for p in (la, ll, ln):
            lp = lp - 0.5 * (p + 0.5) ** 2 - 0.5 * np.log(2 * np.pi)
        return lp - 0.5 * (mu * mu).sum() - K * 0.5 * np.log(2 * np.pi)

    return logp


def _points(K, n, seed):
    """as tests/test_gpu_matrix.py draws them: around a well-conditioned covariance"""
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 3 + K))
    x[:, 0] = -0.2 + 0.3 * rng.normal(size=n)
    x[:, 1] = -0.4 + 0.3 * rng.normal(size=n)
    x[:, 2] = -1.5 + 0.3 * rng.normal(size=n)
    x[:, 3:] = 0.3 + 0.3 * rng.normal(size=(n, K))
    return x


@pytest.mark.parametrize("K,N", [(33, 1), (33, 3), (64, 1), (64, 3), (128, 1), (128, 3)])
def test_host_evaluation_matches_autograd(K, N):
    import torch

    c = mm.gp_rows(K, N).compile(wide_matrices=True)
    logp = _gp_rows_torch(K, N)
    x = _points(K, 4, K + N)
    lp, g = c.logp_and_grad_numpy(x)
    for r in range(4):
        xt = torch.tensor(x[r], requires_grad=True)
        out = logp(xt)
        out.backward()
        print(f"K={K} N={N} point {r}: logp rel {abs(lp[r] - out.item()) / abs(out.item()):.2e}, "
              f"grad rel {np.max(np.abs(g[r] - xt.grad.numpy())) / np.max(np.abs(xt.grad.numpy())):.2e}")
        np.testing.assert_allclose(lp[r], out.item(), rtol=1e-10)
        np.testing.assert_allclose(g[r], xt.grad.numpy(), rtol=1e-10, atol=1e-10 * abs(out.item()))


def _traced_density(n=40):
    """the density of tests/test_matrix_cpu.py::test_a_traced_matrix_past_the_limit_falls_back_to_the_eager_form"""
    import torch

    d2 = torch.as_tensor((np.linspace(0, 4, n)[:, None] - np.linspace(0, 4, n)[None, :]) ** 2)
    y = torch.as_tensor(np.random.default_rng(1).normal(size=n))

    def logp(x):
        C = torch.exp(2 * x[:, 0, None, None]) * torch.exp(-0.5 * d2) + torch.exp(2 * x[:, 1, None, None]) * torch.eye(n, dtype=torch.float64)
        return torch.distributions.MultivariateNormal(torch.zeros(n, dtype=torch.float64), covariance_matrix=C).log_prob(y)

    return logp


def test_traced_matrix_past_32_compiles_with_the_switch():
    import torch

    import nutpie_amd
    from nutpie_amd.torch_trace import trace

    logp = _traced_density()
    c = trace(logp, 2, wide_matrices=True).compile()
    assert "nphip_lw::cholesky<40>(" in c._source and _longest_run_of_literal_stores(c._source) <= 2
    rng = np.random.default_rng(2)
    for _ in range(3):
        x = np.array([[0.1, -1.0]]) + 0.3 * rng.normal(size=(1, 2))
        lp, g = c.logp_and_grad_numpy(x)
        xt = torch.tensor(x, requires_grad=True)
        out = logp(xt)
        out.sum().backward()
        np.testing.assert_allclose(lp[0], out.item(), rtol=1e-10)
        np.testing.assert_allclose(g[0], xt.grad.numpy()[0], rtol=1e-10, atol=1e-10 * abs(out.item()))
    model = nutpie_amd.from_torch_density(2, logp, compile="auto", wide_matrices=True)
    assert "nphip_lw::cholesky<40>" in model._source


@pytest.mark.parametrize("W", [1, 4])
def test_generated_wide_density_compiles_for_gfx950(W):
    from nutpie_amd.density import compile_density, data_layout

    c = mm.gp_rows(128, 1).compile(wide_matrices=True, waves_per_chain=W)
    path = compile_density(c._source, data_layout(c._data), c.n_dim, waves=W)
    assert os.path.exists(path)


def test_gp_example_matches_its_torch_twin():
    import torch

    from nutpie_amd import gp

    t, y = gp.synthetic_gp(100)
    c = gp.compile_gp_regression(t, y)
    assert "nphip_lw::cholesky<100>(" in c._source
    D, logp = gp.gp_regression_torch_density(t, y)
    assert c.n_dim == D == 3
    x = np.array([0.0, -0.2, -1.6]) + 0.3 * np.random.default_rng(7).normal(size=(4, 3))
    lp, g = c.logp_and_grad_numpy(x)
    xt = torch.tensor(x, requires_grad=True)
    out = logp(xt)
    out.sum().backward()
    np.testing.assert_allclose(lp, out.detach().numpy(), rtol=1e-10)
    print("gp example: largest gradient difference", np.max(np.abs(g - xt.grad.numpy())), "of", np.max(np.abs(g)))
    np.testing.assert_allclose(g, xt.grad.numpy(), rtol=1e-10, atol=1e-10 * float(np.abs(out.detach().numpy()).min()))
    # 32 points and fewer: the narrow routines, no option needed
    small = gp.compile_gp_regression(*gp.synthetic_gp(30))
    assert "nphip_la::cholesky<30>(" in small._source and "nphip_lw::" not in small._source
