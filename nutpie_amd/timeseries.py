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
* :func:`local_linear_trend_model` — a structural time series (level + slope, optionally one trigonometric seasonal harmonic) with the
  state summed out by a Kalman filter (``symbolic.kalman_marginal_lpdf``); a share of the steps is missing;
  ``smoothed=True`` reports the smoothed level and its standard deviation (``symbolic.kalman_smoothed_state``), forecasts included.
  Vector: ``[sigma_obs_log__, sigma_level_log__, sigma_slope_log__ (, sigma_seasonal_log__)]``.
* :func:`ar_p_model` — AR(p) in companion form observed with noise: the transition matrix depends on the parameters.
  Vector: ``[rho (p), sigma_log__, tau_log__]``.
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


# --------------------------------------------------------------------------- linear Gaussian state-space models (a Kalman filter)
def _trend_matrices(seasonal_period):
    """(transition, design row, init_cov diagonal) of level + slope (+ one harmonic of ``seasonal_period`` steps)"""
    if seasonal_period is None:
        return np.array([[1.0, 1.0], [0.0, 1.0]]), np.array([1.0, 0.0]), np.array([100.0, 1.0])
    lam = 2.0 * math.pi / float(seasonal_period)
    Tm = np.zeros((4, 4))
    Tm[:2, :2] = [[1.0, 1.0], [0.0, 1.0]]
    Tm[2:, 2:] = [[math.cos(lam), math.sin(lam)], [-math.sin(lam), math.cos(lam)]]
    return Tm, np.array([1.0, 0.0, 1.0, 0.0]), np.array([100.0, 1.0, 25.0, 25.0])


def synthetic_trend(T: int = 200, seasonal_period=None, R: int = 1, missing: float = 0.1, seed: int = 0):
    """(y[R, T], observed[R, T]) drawn from the model itself: sigma_obs 0.5, sigma_level 0.3, sigma_slope 0.05, sigma_seasonal 0.1"""
    rng = np.random.default_rng(20261020 + seed)
    Tm, z, _ = _trend_matrices(seasonal_period)
    scales = np.array([0.3, 0.05, 0.1, 0.1])[:z.size]
    y = np.empty((R, T))
    for r in range(R):
        state = np.array([rng.normal(), 0.1 * rng.normal(), 2.0 * rng.normal(), 2.0 * rng.normal()])[:z.size]
        for t in range(T):
            y[r, t] = z @ state + 0.5 * rng.normal()
            state = Tm @ state + scales * rng.normal(size=z.size)
    observed = (rng.uniform(size=(R, T)) >= missing).astype(np.float64)
    return y, observed


def local_linear_trend_model(T: int = 200, seasonal_period=None, R: int = 1, missing: float = 0.1, seed: int = 0, smoothed: bool = False,
                             forecast: int = 0) -> S.Model:
    """level_{t+1} = level_t + slope_t + sigma_level e, slope_{t+1} = slope_t + sigma_slope e (``seasonal_period``: plus one
    trigonometric harmonic with disturbances sigma_seasonal; the state then has four elements), y_t = level_t (+ seasonal_t) +
    sigma_obs e; every scale ~ HalfNormal(1); the state at t = 0 ~ N(0, diag(100, 1 (, 25, 25))); a share ``missing`` of the steps is
    not observed.  The state is summed out: ``kalman_marginal_lpdf``.  ``R`` > 1: a panel of R series that share the parameters.
    Deterministic ``filtered_level``: the filtered mean of the level at every step (``[R T]``).
    ``smoothed``: also ``smoothed_level`` and ``smoothed_level_sd``, the mean and the standard deviation of the level at every step
    given ALL the observations of its series (``kalman_smoothed_state``): the posterior of the path that was summed out.  Forecasts
    with their variances are the smoothed values on trailing steps with ``observed = 0`` — ``forecast`` appends that many steps to
    every series (the time axis then has ``T + forecast`` elements; their ``y`` is never read)."""
    y, observed = synthetic_trend(T, seasonal_period, R, missing, seed)
    if forecast:
        y, observed = (np.concatenate([v, np.zeros((R, int(forecast)))], axis=1) for v in (y, observed))
        T += int(forecast)
    Tm, z, p0 = _trend_matrices(seasonal_period)
    k = z.size
    m = S.Model()
    names = ["sigma_obs", "sigma_level", "sigma_slope"] + (["sigma_seasonal"] if k == 4 else [])
    scales = [m.param(n, lower=0.0) for n in names]
    for s_ in scales:
        m.add_logp(S.halfnormal_lpdf(s_, 1.0))
    m.dim("state", k)
    if R == 1:
        m.dim("time", T)
        steps, along = "time", None
    else:
        m.dim("series", R)
        m.dim("time", T)
        steps, along = m.product("series", "time").name, "time"
    kk = m.product("state", "state")
    var = [scales[1] * scales[1], scales[2] * scales[2]] + ([scales[3] * scales[3]] * 2 if k == 4 else [])
    Q = S.stack([var[i] if i == j else S.Expr.const(0.0) for i in range(k) for j in range(k)], kk)
    args = dict(design=m.data("design", z, dim="state"), obs_var=scales[0] * scales[0], transition=m.data("transition", Tm.reshape(-1), dim=kk.name),
                state_cov=Q, init_mean=m.data("init_mean", np.zeros(k), dim="state"), init_cov=m.data("init_cov", np.diag(p0).reshape(-1), dim=kk.name),
                observed=m.data("observed", observed.reshape(-1), dim=steps), along=along)
    obs = m.data("y", y.reshape(-1), dim=steps)
    m.add_logp(S.kalman_marginal_lpdf(obs, **args))
    m.deterministic("filtered_level", S.column(S.kalman_filtered_state(obs, **args), 0))
    if smoothed:
        m.deterministic("smoothed_level", S.column(S.kalman_smoothed_state(obs, **args), 0))
        m.deterministic("smoothed_level_sd", S.sqrt(S.column(S.kalman_smoothed_state(obs, variance=True, **args), 0)))
    return m


def _torch_filter(y, observed, Z, h, Tm, Q, a0, P0):
    """the log-likelihood of [chains, R] series by a plain Kalman filter loop in matrix form (torch.autograd differentiates it):
    y, observed [R, T]; Z [T, m] or [m]; h [chains]; Tm, Q, P0 [chains, m, m]; a0 [m]"""
    import torch

    C, (R, T) = h.shape[0], y.shape
    a = a0.expand(C, R, -1)
    P = P0[:, None].expand(C, R, -1, -1)
    total = torch.zeros(C, R, dtype=h.dtype, device=h.device)
    for t in range(T):
        z = Z[t] if Z.dim() == 2 else Z
        v = y[None, :, t] - a @ z
        M = P @ z
        F = h[:, None] + M @ z
        seen = observed[None, :, t]
        total = total - 0.5 * seen * (2.0 * _HALF_LOG_2PI + torch.log(F) + v * v / F)
        K = seen[..., None] * M / F[..., None]
        a = a + K * v[..., None]
        P = P - K[..., :, None] * M[..., None, :]
        a = a @ Tm.transpose(-1, -2)
        P = Tm[:, None] @ P @ Tm.transpose(-1, -2)[:, None] + Q[:, None]
    return total.sum(-1)


def _halfnormal_log(ls):
    """HalfNormal(1) of exp(ls) with the log transform's Jacobian"""
    import torch

    return 0.5 * math.log(2.0 / math.pi) - 0.5 * torch.exp(2.0 * ls) + ls


def local_linear_trend_torch_density(T: int = 200, seasonal_period=None, R: int = 1, missing: float = 0.1, seed: int = 0, device="cpu"):
    """The same log-density as :func:`local_linear_trend_model`, an independent implementation: a plain Python loop over the steps that
    ``torch.autograd`` differentiates.  Returns ``(D, logp)``."""
    import torch

    y_np, obs_np = synthetic_trend(T, seasonal_period, R, missing, seed)
    Tm_np, z_np, p0 = _trend_matrices(seasonal_period)
    k = z_np.size
    dev = torch.device(device) if isinstance(device, str) else torch.device("cuda", device)
    y, observed, Tm, z = (torch.as_tensor(v, device=dev) for v in (y_np, obs_np, Tm_np, z_np))
    P0 = torch.diag(torch.as_tensor(p0, device=dev))
    a0 = torch.zeros(k, dtype=torch.float64, device=dev)

    def logp(x):
        var = torch.exp(2.0 * x)
        diag = [var[:, 1], var[:, 2]] + ([var[:, 3], var[:, 3]] if k == 4 else [])
        Q = torch.diag_embed(torch.stack(diag, dim=-1))
        C = x.shape[0]
        return _halfnormal_log(x).sum(-1) + _torch_filter(y, observed, z, var[:, 0], Tm[None].expand(C, k, k), Q, a0, P0[None].expand(C, k, k))

    return 3 + (k == 4), logp


def local_linear_trend_op_density(T: int = 200, seasonal_period=None, R: int = 1, missing: float = 0.1, seed: int = 0, device="cpu"):
    """The same log-density with :func:`nutpie_amd.torch_trace.kalman_marginal`: what the tracer compiles onto the Kalman filter stage.
    Returns ``(D, logp)``."""
    import torch

    from nutpie_amd.torch_trace import kalman_marginal

    y_np, obs_np = synthetic_trend(T, seasonal_period, R, missing, seed)
    Tm_np, z_np, p0 = _trend_matrices(seasonal_period)
    k = z_np.size
    dev = torch.device(device) if isinstance(device, str) else torch.device("cuda", device)
    y, observed, Tm, z = (torch.as_tensor(v, device=dev) for v in (y_np, obs_np, Tm_np, z_np))
    P0 = torch.diag(torch.as_tensor(p0, device=dev))
    a0 = torch.zeros(k, dtype=torch.float64, device=dev)
    eye = torch.eye(k, dtype=torch.float64, device=dev)

    def logp(x):
        var = torch.exp(2.0 * x)
        diag = [var[:, 1], var[:, 2]] + ([var[:, 3], var[:, 3]] if k == 4 else [])
        Q = torch.stack(diag, dim=-1)[:, :, None] * eye[None]
        ll = kalman_marginal(y[None].expand(x.shape[0], R, T), z, var[:, 0, None, None], Tm, Q[:, None], a0, P0, observed[None])
        return _halfnormal_log(x).sum(-1) + ll.sum(-1)

    return 3 + (k == 4), logp


def synthetic_ar(T: int = 200, p: int = 2, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(20261021 + seed)
    phi = 0.6 / p * np.ones(p)
    x = np.zeros(T + p)
    for t in range(p, T + p):
        x[t] = phi @ x[t - p:t][::-1] + 0.5 * rng.normal()
    return x[p:] + 0.2 * rng.normal(size=T)


def ar_p_model(T: int = 200, p: int = 2, seed: int = 0) -> S.Model:
    """x_t = sum_i phi_i x_{t-i} + sigma e in companion form (the state holds the last p values), y_t = x_t + tau e;
    phi_i = tanh(rho_i) / p (so that sum |phi_i| < 1: stationary), rho ~ Normal(0, 1), sigma, tau ~ HalfNormal(1); the state at t = 0
    ~ N(0, 10 I).  The transition matrix depends on the parameters: the gradient reaches them through the filter's adjoint of it."""
    y = synthetic_ar(T, p, seed)
    m = S.Model()
    m.dim("state", p)
    m.dim("time", T)
    rho = m.param("rho", dim="state")
    sigma, tau = m.param("sigma", lower=0.0), m.param("tau", lower=0.0)
    m.add_logp(S.normal_lpdf(rho, 0.0, 1.0).sum() + S.halfnormal_lpdf(sigma, 1.0) + S.halfnormal_lpdf(tau, 1.0))
    kk = m.product("state", "state")
    phi = S.tanh(rho) / float(p)
    zero, one = S.Expr.const(0.0), S.Expr.const(1.0)
    Tm = S.stack([S.elem(phi, j) if i == 0 else (one if j == i - 1 else zero) for i in range(p) for j in range(p)], kk)
    Q = S.stack([sigma * sigma if i == j == 0 else zero for i in range(p) for j in range(p)], kk)
    e0 = np.zeros(p)
    e0[0] = 1.0
    m.add_logp(S.kalman_marginal_lpdf(m.data("y", y, dim="time"), design=m.data("design", e0, dim="state"), obs_var=tau * tau, transition=Tm,
                                      state_cov=Q, init_mean=0.0, init_cov=m.data("init_cov", (10.0 * np.eye(p)).reshape(-1), dim=kk.name)))
    return m


def ar_p_torch_density(T: int = 200, p: int = 2, seed: int = 0, device="cpu"):
    """The same log-density as :func:`ar_p_model` by a plain Python loop with ``torch.autograd``.  Returns ``(D, logp)``."""
    import torch

    dev = torch.device(device) if isinstance(device, str) else torch.device("cuda", device)
    y = torch.as_tensor(synthetic_ar(T, p, seed), device=dev)[None]
    observed = torch.ones_like(y)
    e0 = torch.zeros(p, dtype=torch.float64, device=dev)
    e0[0] = 1.0
    shift = torch.diag(torch.ones(p - 1, dtype=torch.float64, device=dev), -1)
    P0 = 10.0 * torch.eye(p, dtype=torch.float64, device=dev)

    def logp(x):
        rho, ls, lt = x[:, :p], x[:, p], x[:, p + 1]
        C = x.shape[0]
        Tm = shift[None] + e0[None, :, None] * (torch.tanh(rho) / p)[:, None, :]
        Q = torch.exp(2.0 * ls)[:, None, None] * (e0[:, None] * e0[None, :])[None]
        lp = (-0.5 * rho * rho - _HALF_LOG_2PI).sum(-1) + _halfnormal_log(ls) + _halfnormal_log(lt)
        return lp + _torch_filter(y, observed, e0, torch.exp(2.0 * lt), Tm, Q, torch.zeros_like(e0), P0[None].expand(C, p, p))

    return p + 2, logp
