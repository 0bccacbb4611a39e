"""Time-series models with a latent path or a filtered state, built on the IR's first-order linear recurrence (``symbolic.linear_recurrence``
/ ``cumsum``): each as a symbolic model and as a batched torch log-density of the same flat vector (its twin: eager
through ``from_torchfunc``, or traced with :func:`nutpie_amd.torch_trace.trace`).  The data are synthetic, drawn with a fixed seed.

* :func:`stochastic_volatility_model` — PyMC's stochastic-volatility example, non-centred: the log-variance ``h = mu + cumsum(sigma z)``
  is a Gaussian random walk, ``returns ~ StudentT(nu, 0, exp(h / 2))``; reports ``volatility = exp(h / 2)``.
  Unconstrained vector: ``[mu, sigma_log__, nu_log__, z (T)]``.
* :func:`garch11_model` — GARCH(1, 1): ``y_t ~ Normal(mu, s_t)``, ``s_t^2 = omega + alpha (y_{t-1} - mu)^2 + beta s_{t-1}^2`` with
  ``s_0^2`` the sample variance; ``omega > 0``, ``alpha, beta`` in (0, 1).  Vector: ``[mu, omega_log__, alpha_interval__, beta_interval__]``.
* :func:`ar1_latent_model` — a non-centred stationary AR(1) latent state ``x_t = phi x_{t-1} + sigma z_t`` (``x_0 = sigma z_0 /
  sqrt(1 - phi^2)``) observed with Normal noise ``tau``.  Vector: ``[phi_interval__, sigma_log__, tau_log__, z (T)]``.
* :func:`regime_switching_model` — a Gaussian hidden Markov model (regime switching): the discrete state is summed out by the forward
  algorithm (``symbolic.hmm_marginal_lpdf``); ordered state means, one scale, a transition matrix of simplex rows.
  Vector: ``[mu_ordered__ (K), sigma_log__, P_0_simplex__ (K - 1), ..., P_{K-1}_simplex__ (K - 1)]``.
"""

from __future__ import annotations

import math

import numpy as np

from nutpie_amd import symbolic as S

_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


# --------------------------------------------------------------------------- synthetic data
def synthetic_returns(n: int = 2000, mu: float = -9.0, sigma: float = 0.1, nu: float = 8.0, seed: int = 20261016) -> np.ndarray:
    """daily-looking returns from the stochastic-volatility model itself"""
    rng = np.random.default_rng(seed)
    h = mu + np.cumsum(sigma * rng.normal(size=n))
    return np.exp(h / 2.0) * rng.standard_t(nu, size=n)


def synthetic_garch(n: int = 1000, mu: float = 0.05, omega: float = 0.1, alpha: float = 0.2, beta: float = 0.7, seed: int = 20261017) -> np.ndarray:
    rng = np.random.default_rng(seed)
    y = np.empty(n)
    s2, e_prev = omega / (1.0 - alpha - beta), 0.0
    for t in range(n):
        if t:
            s2 = omega + alpha * e_prev * e_prev + beta * s2
        e_prev = math.sqrt(s2) * rng.normal()
        y[t] = mu + e_prev
    return y


def synthetic_ar1(n: int = 500, phi: float = 0.8, sigma: float = 0.5, tau: float = 0.3, seed: int = 20261018) -> np.ndarray:
    rng = np.random.default_rng(seed)
    x = np.empty(n)
    x[0] = sigma / math.sqrt(1.0 - phi * phi) * rng.normal()
    for t in range(1, n):
        x[t] = phi * x[t - 1] + sigma * rng.normal()
    return x + tau * rng.normal(size=n)


# --------------------------------------------------------------------------- stochastic volatility
def stochastic_volatility_model(returns=None) -> S.Model:
    """mu ~ Normal(0, 10), sigma ~ Exponential(10), nu ~ Exponential(0.1), z ~ Normal(0, 1) on ``time``; h = mu + cumsum(sigma z);
    returns ~ StudentT(nu, 0, exp(h / 2)).  Deterministic ``volatility`` = exp(h / 2)."""
    y = np.asarray(synthetic_returns() if returns is None else returns, dtype=np.float64)
    m = S.Model()
    m.dim("time", y.size)
    mu = m.param("mu")
    sigma = m.param("sigma", lower=0.0)
    nu = m.param("nu", lower=0.0)
    z = m.param("z", dim="time")
    r = m.data("returns", y, dim="time")
    m.add_logp(S.normal_lpdf(mu, 0.0, 10.0))
    m.add_logp(S.exponential_lpdf(sigma, 10.0))
    m.add_logp(S.exponential_lpdf(nu, 0.1))
    m.add_logp(S.normal_lpdf(z, 0.0, 1.0).sum())
    h = mu + S.cumsum(sigma * z)
    m.add_logp(S.student_t_lpdf(r, nu, 0.0, S.exp(0.5 * h)).sum())
    m.deterministic("volatility", S.exp(0.5 * h))
    return m


def _student_t(x, nu, scale):
    import torch

    z = x / scale
    return (torch.lgamma(0.5 * (nu + 1.0)) - torch.lgamma(0.5 * nu) - 0.5 * torch.log(nu * math.pi) - torch.log(scale)
            - 0.5 * (nu + 1.0) * torch.log1p(z * z / nu))


def stochastic_volatility_torch_density(returns=None, device="cpu"):
    """The same log-density as :func:`stochastic_volatility_model` as a batched torch function (``torch.cumsum`` for the walk).
    Returns ``(D, logp)``."""
    import torch

    y_np = np.asarray(synthetic_returns() if returns is None else returns, dtype=np.float64)
    dev = torch.device(device) if isinstance(device, str) else torch.device("cuda", device)
    y = torch.as_tensor(y_np, device=dev)

    def logp(x):
        mu, ls, lnu, z = x[:, 0], x[:, 1], x[:, 2], x[:, 3:]
        sigma, nu = ls.exp(), lnu.exp()
        lp = -0.5 * (mu / 10.0) ** 2 - math.log(10.0) - _HALF_LOG_2PI
        lp = lp + math.log(10.0) - 10.0 * sigma + ls + math.log(0.1) - 0.1 * nu + lnu
        lp = lp - 0.5 * (z * z).sum(-1) - z.shape[-1] * _HALF_LOG_2PI
        h = mu[:, None] + torch.cumsum(sigma[:, None] * z, dim=-1)
        return lp + _student_t(y, nu[:, None], torch.exp(0.5 * h)).sum(-1)

    return 3 + y_np.size, logp


# --------------------------------------------------------------------------- GARCH(1, 1)
def garch11_model(y=None) -> S.Model:
    """mu ~ Normal(0, 1), omega ~ HalfNormal(1), alpha, beta ~ Uniform(0, 1); the variance filter is one scan over t = 1 .. T-1
    (a = beta, b_t = omega + alpha (y_{t-1} - mu)^2, init = the sample variance s_0^2); y_t ~ Normal(mu, s_t)."""
    y = np.asarray(synthetic_garch() if y is None else y, dtype=np.float64)
    var0 = float(np.var(y))
    m = S.Model()
    m.dim("t1", y.size - 1)
    mu = m.param("mu")
    omega = m.param("omega", lower=0.0)
    alpha = m.param("alpha", lower=0.0, upper=1.0)
    beta = m.param("beta", lower=0.0, upper=1.0)
    y_cur = m.data("y_cur", y[1:], dim="t1")
    y_prev = m.data("y_prev", y[:-1], dim="t1")
    m.add_logp(S.normal_lpdf(mu, 0.0, 1.0))
    m.add_logp(S.halfnormal_lpdf(omega, 1.0))
    e = y_prev - mu
    s2 = S.linear_recurrence(beta, omega + alpha * (e * e), init=var0)
    m.add_logp(S.normal_lpdf(float(y[0]), mu, math.sqrt(var0)))
    m.add_logp(S.normal_lpdf(y_cur, mu, S.sqrt(s2)).sum())
    return m


def garch11_torch_density(y=None, device="cpu"):
    """The same log-density as :func:`garch11_model` with :func:`nutpie_amd.torch_trace.linear_recurrence`.  Returns ``(D, logp)``."""
    import torch

    from nutpie_amd.torch_trace import linear_recurrence

    y_np = np.asarray(synthetic_garch() if y is None else y, dtype=np.float64)
    var0 = float(np.var(y_np))
    dev = torch.device(device) if isinstance(device, str) else torch.device("cuda", device)
    yc, yp = torch.as_tensor(y_np[1:], device=dev), torch.as_tensor(y_np[:-1], device=dev)
    y0 = float(y_np[0])

    def logp(x):
        mu, lo, ra, rb = x[:, 0], x[:, 1], x[:, 2], x[:, 3]
        omega, alpha, beta = lo.exp(), torch.sigmoid(ra), torch.sigmoid(rb)
        lp = -0.5 * mu * mu - _HALF_LOG_2PI + 0.5 * math.log(2.0 / math.pi) - 0.5 * omega * omega + lo
        lp = lp - torch.nn.functional.softplus(ra) - torch.nn.functional.softplus(-ra) - torch.nn.functional.softplus(rb) - torch.nn.functional.softplus(-rb)
        lp = lp - 0.5 * (y0 - mu) ** 2 / var0 - 0.5 * math.log(var0) - _HALF_LOG_2PI
        e = yp - mu[:, None]
        s2 = linear_recurrence(beta[:, None], omega[:, None] + alpha[:, None] * e * e, var0)
        r = yc - mu[:, None]
        return lp - (0.5 * r * r / s2 + 0.5 * torch.log(s2)).sum(-1) - yc.shape[0] * _HALF_LOG_2PI

    return 4, logp


# --------------------------------------------------------------------------- AR(1) latent state
def ar1_latent_model(y=None) -> S.Model:
    """phi ~ Uniform(-1, 1), sigma ~ HalfNormal(1), tau ~ HalfNormal(1), z ~ Normal(0, 1) on ``time``; x = linear_recurrence(phi,
    sigma z with z_0 scaled by 1 / sqrt(1 - phi^2)); y ~ Normal(x, tau).  Deterministic ``latent`` = x."""
    y = np.asarray(synthetic_ar1() if y is None else y, dtype=np.float64)
    m = S.Model()
    time = m.dim("time", y.size)
    phi = m.param("phi", lower=-1.0, upper=1.0)
    sigma = m.param("sigma", lower=0.0)
    tau = m.param("tau", lower=0.0)
    z = m.param("z", dim="time")
    obs = m.data("y", y, dim="time")
    m.add_logp(S.uniform_lpdf(phi, -1.0, 1.0) + S.halfnormal_lpdf(sigma, 1.0) + S.halfnormal_lpdf(tau, 1.0))
    m.add_logp(S.normal_lpdf(z, 0.0, 1.0).sum())
    innov = sigma * z * S.where_lt(time, 1, 1.0 / S.sqrt(1.0 - phi * phi), 1.0)
    x = S.linear_recurrence(phi, innov)
    m.add_logp(S.normal_lpdf(obs, x, tau).sum())
    m.deterministic("latent", x)
    return m


def ar1_latent_torch_density(y=None, device="cpu"):
    """The same log-density as :func:`ar1_latent_model`.  Returns ``(D, logp)``."""
    import torch

    from nutpie_amd.torch_trace import linear_recurrence

    y_np = np.asarray(synthetic_ar1() if y is None else y, dtype=np.float64)
    dev = torch.device(device) if isinstance(device, str) else torch.device("cuda", device)
    y = torch.as_tensor(y_np, device=dev)

    def logp(x):
        rp, ls, lt, z = x[:, 0], x[:, 1], x[:, 2], x[:, 3:]
        phi, sigma, tau = 2.0 * torch.sigmoid(rp) - 1.0, ls.exp(), lt.exp()
        lp = math.log(2.0) - torch.nn.functional.softplus(rp) - torch.nn.functional.softplus(-rp) - math.log(2.0)
        lp = lp + math.log(2.0 / math.pi) - 0.5 * sigma * sigma + ls - 0.5 * tau * tau + lt
        lp = lp - 0.5 * (z * z).sum(-1) - z.shape[-1] * _HALF_LOG_2PI
        innov = sigma[:, None] * z
        innov = torch.cat([innov[:, :1] / torch.sqrt(1.0 - phi * phi)[:, None], innov[:, 1:]], dim=-1)
        lat = linear_recurrence(phi[:, None], innov, 0.0)
        r = (y - lat) / tau[:, None]
        return lp - 0.5 * (r * r).sum(-1) - y.shape[0] * (lt + _HALF_LOG_2PI)

    return 3 + y_np.size, logp


# --------------------------------------------------------------------------- regime switching (a Gaussian hidden Markov model)
def synthetic_regimes(T: int = 200, K: int = 2, R: int = 1, stay: float = 0.9, sigma: float = 0.7, seed: int = 20261019) -> np.ndarray:
    """R series of T observations from a sticky K-state chain (it keeps its state with probability ``stay``) with state means
    ``3 (k - (K - 1) / 2)`` and Normal noise ``sigma``"""
    rng = np.random.default_rng(seed)
    means = 3.0 * (np.arange(K) - 0.5 * (K - 1))
    y = np.empty((R, T))
    for r in range(R):
        z = rng.integers(K)
        for t in range(T):
            if t and K > 1 and rng.uniform() > stay:
                z = (z + 1 + rng.integers(K - 1)) % K
            y[r, t] = means[z] + sigma * rng.normal()
    return y


_REGIME_CONCENTRATION = 2.0


def regime_switching_model(T: int = 200, K: int = 2, seed: int = 20261019, R: int = 1, y=None) -> S.Model:
    """mu ~ Normal(0, 5) on the K states, ordered (the labels cannot switch); sigma ~ HalfNormal(2); every row of the transition
    matrix P ~ Dirichlet(2) (``Model.transition_matrix``); the initial distribution uniform and constant; y_t ~ Normal(mu[z_t], sigma)
    with the states z summed out: ``hmm_marginal_lpdf``.  ``R`` > 1: a panel of R independent series that share the parameters.
    Deterministic ``state_prob``: the smoothed probability of every state at every step (``[R T, K]``)."""
    y = np.asarray(synthetic_regimes(T, K, R, seed=seed) if y is None else y, dtype=np.float64).reshape(R, T)
    m = S.Model()
    mu = m.param("mu", dim="P_k", size=K, ordered=True, initval=3.0 * (np.arange(K) - 0.5 * (K - 1)))
    sigma = m.param("sigma", lower=0.0)
    P = m.transition_matrix("P", K, concentration=_REGIME_CONCENTRATION)
    m.add_logp(S.normal_lpdf(mu, 0.0, 5.0).sum() + S.halfnormal_lpdf(sigma, 2.0))
    if R == 1:
        m.dim("time", T)
        steps, along = "time", None
    else:
        m.dim("series", R)
        m.dim("time", T)
        steps, along = m.product("series", "time").name, "time"
    obs = m.data("y", y.reshape(-1), dim=steps)
    log_emission = S.normal_lpdf(m.broadcast(obs, steps, "P_k"), m.broadcast(mu, steps, "P_k"), sigma)
    pi = m.data("initial", np.full(K, 1.0 / K), dim="P_k")
    m.add_logp(S.hmm_marginal_lpdf(log_emission, P, pi, along=along))
    m.deterministic("state_prob", S.hmm_state_prob(log_emission, P, pi, along=along))
    return m


def regime_switching_torch_density(T: int = 200, K: int = 2, seed: int = 20261019, R: int = 1, y=None, device="cpu"):
    """The same log-density as :func:`regime_switching_model` with :func:`nutpie_amd.torch_trace.hmm_marginal`.  Returns ``(D, logp)``."""
    import torch

    from nutpie_amd.torch_trace import hmm_marginal

    y_np = np.asarray(synthetic_regimes(T, K, R, seed=seed) if y is None else y, dtype=np.float64).reshape(R, T)
    dev = torch.device(device) if isinstance(device, str) else torch.device("cuda", device)
    obs = torch.as_tensor(y_np, device=dev)
    conc = _REGIME_CONCENTRATION
    dirichlet_const = math.lgamma(K * conc) - K * math.lgamma(conc)

    def logp(x):
        raw_mu, ls, raw_p = x[:, :K], x[:, K], x[:, K + 1:].reshape(-1, K, K - 1)
        mu = torch.cat([raw_mu[:, :1], raw_mu[:, :1] + torch.cumsum(torch.exp(raw_mu[:, 1:]), dim=-1)], dim=-1) if K > 1 else raw_mu
        sigma = ls.exp()
        lp = raw_mu[:, 1:].sum(-1) - (0.5 * (mu / 5.0) ** 2).sum(-1) - K * (math.log(5.0) + _HALF_LOG_2PI)
        lp = lp + 0.5 * math.log(2.0 / math.pi) - math.log(2.0) - 0.5 * (sigma / 2.0) ** 2 + ls
        # the simplex transform of every row (the softmax of the zero-sum extension of its free values) and its Jacobian
        s = raw_p.sum(-1, keepdim=True)
        z = torch.cat([raw_p + s, torch.zeros_like(s)], dim=-1)
        lse = torch.logsumexp(z, dim=-1, keepdim=True)
        log_rows = z - lse
        lp = lp + (math.log(K) + K * s - K * lse).sum((-1, -2)) + (conc - 1.0) * log_rows.sum((-1, -2)) + K * dirichlet_const
        r = (obs[None, :, :, None] - mu[:, None, None, :]) / sigma[:, None, None, None]
        log_emission = -0.5 * r * r - ls[:, None, None, None] - _HALF_LOG_2PI
        initial = torch.full((K,), 1.0 / K, dtype=x.dtype, device=x.device)
        return lp + hmm_marginal(log_emission, torch.exp(log_rows)[:, None], initial).sum(-1)

    return K + 1 + K * (K - 1), logp
