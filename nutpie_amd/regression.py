"""Regressions with a wide design matrix, built on the IR's data-matrix stage (``Matrix @`` with 64 columns or more, ``Matrix.T @``;
``csrc/chain_matvec.h``): each as a symbolic model and as a batched torch log-density of the same flat vector (its
twin: eager through ``from_torchfunc``, or traced with :func:`nutpie_amd.torch_trace.trace`).  The data are synthetic, drawn with a
fixed seed.

* :func:`logistic_regression_model` — ``y ~ Bernoulli(logit = a + X beta)``, ``a, beta ~ Normal(0, 1)``.
  Unconstrained vector: ``[a, beta (k)]``.
* :func:`horseshoe_regression_model` — the regularised horseshoe (Piironen & Vehtari 2017): ``beta = z tau lambda~`` with
  ``lambda~^2 = c2 lambda^2 / (c2 + tau^2 lambda^2)``, ``y ~ Normal(a + X beta, sigma)``: the stage's operand is a computed vector, its
  adjoint flows on through element-wise code.  Vector: ``[a, sigma_log__, tau_log__, c2_log__, z (k), lam_log__ (k)]``.
* :func:`softmax_regression_model` — ``y ~ Categorical(softmax(b0 + X B))`` with ``B`` on ``product(coef, class)``: one product with R =
  ``n_classes`` right-hand sides (``times<K, R>``), the log-softmax written on the columns of the n x R result (``symbolic.column``).
  Vector: ``[B (k x R, row-major), b0 (R)]``.
* :func:`linear_regression_model` — ``y ~ Normal(a + X beta, sigma)`` with ``sigma`` known and Normal priors: the posterior is a
  Gaussian in closed form (:func:`linear_regression_posterior`), which is what the sampler's law is tested against.

``stage`` is handed to ``Model.matrix``: None lowers by the number of columns, True / False force the device routine resp. the sum
over the columns.
"""

from __future__ import annotations

import math

import numpy as np

from nutpie_amd import symbolic as S

_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


# --------------------------------------------------------------------------- synthetic data
def synthetic_design(n: int = 2000, k: int = 200, seed: int = 20261019) -> tuple[np.ndarray, np.ndarray]:
    """``(X, eta)``: an n x k design matrix of standardised, mildly correlated predictors (scaled by 1 / sqrt(k): the linear predictor
    of unit coefficients has unit variance) and the linear predictor ``X beta`` of a sparse truth (every tenth coefficient is 2)."""
    rng = np.random.default_rng(seed)
    common = rng.normal(size=(n, 1))
    X = (rng.normal(size=(n, k)) + 0.3 * common) / math.sqrt(1.09 * k)
    beta = np.where(np.arange(k) % 10 == 0, 2.0, 0.0)
    return X, X @ beta


def synthetic_binary(eta: np.ndarray, seed: int = 20261020) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return (rng.random(eta.size) < 1.0 / (1.0 + np.exp(-(0.3 + eta)))).astype(np.float64)


def synthetic_response(eta: np.ndarray, sigma: float = 0.5, seed: int = 20261021) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return 0.3 + eta + sigma * rng.normal(size=eta.size)


def _default(X, y, make):
    if X is None:
        X, eta = synthetic_design()
        y = make(eta)
    return np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)


def _torch_data(X, y, device):
    import torch

    dev = torch.device(device) if isinstance(device, str) else torch.device("cuda", device)
    return torch.as_tensor(X, device=dev), torch.as_tensor(y, device=dev)


# --------------------------------------------------------------------------- logistic regression
def logistic_regression_model(X=None, y=None, stage: bool | None = None) -> S.Model:
    """a ~ Normal(0, 1), beta ~ Normal(0, 1) on ``coef``; y ~ Bernoulli(logit = a + X beta)."""
    X, y = _default(X, y, synthetic_binary)
    m = S.Model()
    a = m.param("a")
    beta = m.param("beta", dim="coef", size=X.shape[1])
    Xm = m.matrix("X", X, dim="obs", cols="coef", stage=stage)
    yv = m.data("y", y, dim="obs")
    m.add_logp(S.normal_lpdf(a, 0.0, 1.0))
    m.add_logp(S.normal_lpdf(beta, 0.0, 1.0).sum())
    m.add_logp(S.bernoulli_logit_lpmf(yv, a + Xm @ beta).sum())
    return m


def logistic_regression_torch_density(X=None, y=None, device="cpu"):
    """The same log-density as :func:`logistic_regression_model` as a batched torch function.  Returns ``(D, logp)``."""
    import torch

    X, y = _default(X, y, synthetic_binary)
    k = X.shape[1]
    Xt, yt = _torch_data(X, y, device)

    def logp(x):
        a, beta = x[:, 0], x[:, 1:]
        lp = -0.5 * a * a - _HALF_LOG_2PI - 0.5 * (beta * beta).sum(-1) - k * _HALF_LOG_2PI
        eta = a[:, None] + beta @ Xt.T
        return lp + (yt * eta - torch.nn.functional.softplus(eta)).sum(-1)

    return 1 + k, logp


# --------------------------------------------------------------------------- regularised horseshoe
def horseshoe_regression_model(X=None, y=None, tau0: float = 0.1, stage: bool | None = None) -> S.Model:
    """a ~ Normal(0, 1), sigma ~ HalfNormal(1), tau ~ HalfCauchy(tau0), c2 ~ InverseGamma(2, 2), z ~ Normal(0, 1) and
    lam ~ HalfCauchy(1) on ``coef``; beta = z tau lam sqrt(c2 / (c2 + tau^2 lam^2)); y ~ Normal(a + X beta, sigma).  Reports ``beta``."""
    X, y = _default(X, y, synthetic_response)
    k = X.shape[1]
    m = S.Model()
    a = m.param("a")
    sigma = m.param("sigma", lower=0.0)
    tau = m.param("tau", lower=0.0)
    c2 = m.param("c2", lower=0.0)
    z = m.param("z", dim="coef", size=k)
    lam = m.param("lam", dim="coef", lower=0.0)
    Xm = m.matrix("X", X, dim="obs", cols="coef", stage=stage)
    yv = m.data("y", y, dim="obs")
    m.add_logp(S.normal_lpdf(a, 0.0, 1.0))
    m.add_logp(S.halfnormal_lpdf(sigma, 1.0))
    m.add_logp(S.halfcauchy_lpdf(tau, tau0))
    m.add_logp(S.inverse_gamma_lpdf(c2, 2.0, 2.0))
    m.add_logp(S.normal_lpdf(z, 0.0, 1.0).sum())
    m.add_logp(S.halfcauchy_lpdf(lam, 1.0).sum())
    tl = tau * lam
    beta = z * tl * S.sqrt(c2 / (c2 + tl * tl))
    m.add_logp(S.normal_lpdf(yv, a + Xm @ beta, sigma).sum())
    m.deterministic("beta", beta)
    return m


def horseshoe_regression_torch_density(X=None, y=None, tau0: float = 0.1, device="cpu"):
    """The same log-density as :func:`horseshoe_regression_model` (log transforms and their Jacobians written out).  ``(D, logp)``."""
    import torch

    X, y = _default(X, y, synthetic_response)
    n, k = X.shape
    Xt, yt = _torch_data(X, y, device)
    log_2_pi = math.log(2.0 / math.pi)

    def logp(x):
        a, ls, lt, lc = x[:, 0], x[:, 1], x[:, 2], x[:, 3]
        z, ll = x[:, 4:4 + k], x[:, 4 + k:]
        sigma, tau, c2, lam = ls.exp(), lt.exp(), lc.exp(), ll.exp()
        lp = -0.5 * a * a - _HALF_LOG_2PI
        lp = lp - 0.5 * sigma * sigma + 0.5 * log_2_pi + ls
        lp = lp + log_2_pi - math.log(tau0) - torch.log1p((tau / tau0) ** 2) + lt
        lp = lp + 2.0 * math.log(2.0) - math.lgamma(2.0) - 3.0 * lc - 2.0 / c2 + lc
        lp = lp - 0.5 * (z * z).sum(-1) - k * _HALF_LOG_2PI
        lp = lp + (log_2_pi - torch.log1p(lam * lam) + ll).sum(-1)
        tl = tau[:, None] * lam
        beta = z * tl * torch.sqrt(c2[:, None] / (c2[:, None] + tl * tl))
        r = (yt - (a[:, None] + beta @ Xt.T)) / sigma[:, None]
        return lp - 0.5 * (r * r).sum(-1) - n * (ls + _HALF_LOG_2PI)

    return 4 + 2 * k, logp


# --------------------------------------------------------------------------- softmax regression
def synthetic_classes(X: np.ndarray, n_classes: int = 4, seed: int = 20261022) -> np.ndarray:
    rng = np.random.default_rng(seed)
    eta = 3.0 * X @ rng.normal(size=(X.shape[1], n_classes))
    p = np.exp(eta - eta.max(1, keepdims=True))
    return (rng.random((len(X), 1)) > np.cumsum(p / p.sum(1, keepdims=True), axis=1)).sum(1).clip(0, n_classes - 1)


def softmax_regression_model(X=None, y=None, n_classes: int = 4) -> S.Model:
    """B ~ Normal(0, 1) on ``product(coef, class)``, b0 ~ Normal(0, 1) on ``class``; y ~ Categorical(softmax(b0 + X B)) — ``y`` the class
    of every observation, 0 .. n_classes - 1.  ``X @ B`` is one product with n_classes right-hand sides; the log-sum-exp over the classes is
    element-wise code on the observations, over the columns of the result, shifted by their largest."""
    if X is None:
        X, _ = synthetic_design()
        y = synthetic_classes(X, n_classes)
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.int64)
    R = int(n_classes)
    m = S.Model()
    m.dim("coef", X.shape[1])
    m.dim("class", R)
    B = m.param("B", dims=("coef", "class"))
    b0 = m.param("b0", dim="class")
    eta = m.matrix("X", X, dim="obs", cols="coef") @ B                 # n x R, on product(obs, class)
    onehot = m.data("y_onehot", np.eye(R)[y].reshape(-1), dim=eta.dim.name)
    cols = [S.column(eta, r) + S.elem(b0, r) for r in range(R)]
    top = cols[0]
    for c in cols[1:]:
        top = S.select(c - top, c, top)
    total = picked = None
    for r, c in enumerate(cols):
        e, p = S.exp(c - top), S.column(onehot, r) * c
        total, picked = (e, p) if total is None else (total + e, picked + p)
    m.add_logp(S.normal_lpdf(B, 0.0, 1.0).sum() + S.normal_lpdf(b0, 0.0, 1.0).sum())
    m.add_logp((picked - S.log(total) - top).sum())
    return m


def softmax_regression_torch_density(X=None, y=None, n_classes: int = 4, device="cpu"):
    """The same log-density as :func:`softmax_regression_model` as a batched torch function.  Returns ``(D, logp)``."""
    import torch

    if X is None:
        X, _ = synthetic_design()
        y = synthetic_classes(X, n_classes)
    X = np.asarray(X, dtype=np.float64)
    k, R = X.shape[1], int(n_classes)
    Xt, _ = _torch_data(X, np.zeros(1), device)
    yt = torch.as_tensor(np.asarray(y, dtype=np.int64), device=Xt.device)

    def logp(x):
        B, b0 = x[:, :k * R].reshape(-1, k, R), x[:, k * R:]
        lp = -0.5 * (x * x).sum(-1) - (k * R + R) * _HALF_LOG_2PI
        eta = Xt @ B + b0[:, None, :]
        return lp + torch.log_softmax(eta, -1)[:, torch.arange(len(yt), device=yt.device), yt].sum(-1)

    return k * R + R, logp


# --------------------------------------------------------------------------- Gaussian linear regression, sigma known
def linear_regression_model(X=None, y=None, sigma: float = 0.5, prior_sd: float = 1.0, stage: bool | None = None) -> S.Model:
    """a ~ Normal(0, prior_sd), beta ~ Normal(0, prior_sd) on ``coef``; y ~ Normal(a + X beta, sigma) with ``sigma`` known."""
    X, y = _default(X, y, synthetic_response)
    m = S.Model()
    a = m.param("a")
    beta = m.param("beta", dim="coef", size=X.shape[1])
    Xm = m.matrix("X", X, dim="obs", cols="coef", stage=stage)
    yv = m.data("y", y, dim="obs")
    m.add_logp(S.normal_lpdf(a, 0.0, prior_sd))
    m.add_logp(S.normal_lpdf(beta, 0.0, prior_sd).sum())
    m.add_logp(S.normal_lpdf(yv, a + Xm @ beta, sigma).sum())
    return m


def linear_regression_posterior(X, y, sigma: float = 0.5, prior_sd: float = 1.0) -> tuple[np.ndarray, np.ndarray]:
    """Mean and covariance of ``[a, beta]`` under :func:`linear_regression_model`: ``S = (Z^T Z / sigma^2 + I / prior_sd^2)^-1``,
    ``m = S Z^T y / sigma^2`` with ``Z = [1, X]``."""
    Z = np.concatenate([np.ones((len(y), 1)), np.asarray(X, dtype=np.float64)], axis=1)
    cov = np.linalg.inv(Z.T @ Z / sigma ** 2 + np.eye(Z.shape[1]) / prior_sd ** 2)
    return cov @ (Z.T @ np.asarray(y, dtype=np.float64)) / sigma ** 2, cov
