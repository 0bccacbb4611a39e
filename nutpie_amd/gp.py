"""Exact Gaussian-process regression on up to 128 points, built on the IR's matrix stages (``cholesky`` / ``solve_lower``; the panel
routines of ``csrc/wide_chain_linalg.h`` above 32 points): as a symbolic model and as a batched torch log-density of the same
flat vector (its twin: eager through ``from_torchfunc``, or traced with ``from_torch_density(..., wide_matrices=True)``).

``y ~ MvNormal(0, C)``, ``C[i][j] = amp^2 exp(-(t_i - t_j)^2 / (2 ls^2)) + noise^2 [i = j]``: the marginal likelihood of a squared-exponential
kernel, one right-hand side; ``log amp, log ls, log noise ~ Normal(0, 1)``.  Unconstrained vector: ``[log_amp, log_ls, log_noise]``.
"""

from __future__ import annotations

import math

import numpy as np

from nutpie_amd import symbolic as S
from nutpie_amd.stage_families.linalg import MAX_MATRIX

_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def synthetic_gp(n: int = 100, length_scale: float = 0.8, amplitude: float = 1.0, noise: float = 0.2, seed: int = 20261020) -> tuple[np.ndarray, np.ndarray]:
    """``(t, y)``: ``n`` points on [0, 5] and one draw of the process observed with noise."""
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 5.0, n)
    cov = amplitude**2 * np.exp(-0.5 * (t[:, None] - t[None, :]) ** 2 / length_scale**2) + 1e-10 * np.eye(n)
    return t, np.linalg.cholesky(cov) @ rng.normal(size=n) + noise * rng.normal(size=n)


def _default(t, y):
    if t is None:
        t, y = synthetic_gp()
    t, y = np.asarray(t, dtype=np.float64).reshape(-1), np.asarray(y, dtype=np.float64).reshape(-1)
    if t.size != y.size:
        raise ValueError("gp regression: t and y have one value per point")
    return t, y


def gp_regression_model(t=None, y=None) -> S.Model:
    """The marginal likelihood as a symbolic model.  ``compile_gp_regression`` compiles it with the option its size needs."""
    t, y = _default(t, y)
    n = t.size
    m = S.Model()
    m.dim("pt", n)
    kk = m.product("pt", "pt")
    log_amp, log_ls, log_noise = m.param("log_amp"), m.param("log_ls"), m.param("log_noise")
    D2 = m.data("d2", ((t[:, None] - t[None, :]) ** 2).reshape(-1), dim=kk.name)
    eye = m.data("eye", np.eye(n).reshape(-1), dim=kk.name)
    Y = m.data("y", y, dim="pt")
    C = S.exp(2.0 * log_amp) * S.exp(-0.5 * D2 * S.exp(-2.0 * log_ls)) + S.exp(2.0 * log_noise) * eye
    m.add_logp(S.mvnormal_lpdf(Y, 0.0, cov=C))
    for p in (log_amp, log_ls, log_noise):
        m.add_logp(S.normal_lpdf(p, 0.0, 1.0))
    m.deterministic("length_scale", S.exp(log_ls))
    return m


def compile_gp_regression(t=None, y=None, **kw):
    """:func:`gp_regression_model` compiled: above 32 points with ``wide_matrices=True`` (other keywords go to ``Model.compile``)."""
    m = gp_regression_model(t, y)
    kw.setdefault("wide_matrices", m._dims["pt"].size > MAX_MATRIX)
    return m.compile(**kw)


def gp_regression_torch_density(t=None, y=None, device="cpu"):
    """The same log-density as :func:`gp_regression_model` as a batched torch function (one batched Cholesky over all chains).
    Returns ``(D, logp)``."""
    import torch

    t, y = _default(t, y)
    n = t.size
    dev = torch.device(device) if isinstance(device, str) else torch.device("cuda", device)
    d2 = torch.as_tensor((t[:, None] - t[None, :]) ** 2, device=dev)
    yt = torch.as_tensor(y, device=dev)
    eye = torch.eye(n, dtype=torch.float64, device=dev)
    zero = torch.zeros(n, dtype=torch.float64, device=dev)

    def logp(x):
        C = torch.exp(2 * x[:, 0, None, None]) * torch.exp(-0.5 * d2 * torch.exp(-2 * x[:, 1, None, None])) + torch.exp(2 * x[:, 2, None, None]) * eye
        # (cholesky_ex: a covariance that is not positive definite — a far corner early in the warm-up — gives NaN, an impossible point,
        #  where torch.linalg.cholesky would raise out of the sampler)
        L, info = torch.linalg.cholesky_ex(C)
        lp = torch.distributions.MultivariateNormal(zero, scale_tril=L, validate_args=False).log_prob(yt)
        lp = torch.where(info > 0, torch.full_like(lp, float("nan")), lp)
        return lp - 0.5 * (x * x).sum(-1) - 3 * _HALF_LOG_2PI

    return 3, logp
