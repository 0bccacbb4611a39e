"""Models with per-chain dense matrices (the symbolic IR's cholesky / solve_lower stages), shared by the CPU and GPU tests."""
from __future__ import annotations

import math

import numpy as np

from nutpie_amd import symbolic as S


def gp_rows(K: int, N: int, seed: int = 0, factor_deterministic: bool = False):
    """N independent draws of a K-point Gaussian process (squared-exponential kernel of amplitude, length-scale and noise: three log
    parameters) around a mean vector ``mu`` (K parameters): the covariance, its factor and both solves depend on parameters."""
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 3.0, K)
    d2 = (t[:, None] - t[None, :]) ** 2
    cov = 0.8**2 * np.exp(-0.5 * d2 / 0.7**2) + 0.1**2 * np.eye(K)
    y = np.linalg.cholesky(cov) @ rng.normal(size=(K, N)) + 0.3       # K x N: every column one draw
    m = S.Model()
    m.dim("k", K)
    m.dim("obs", N)
    kk = m.product("k", "k")
    kn = m.product("k", "obs")
    log_amp = m.param("log_amp")
    log_ls = m.param("log_ls")
    log_noise = m.param("log_noise")
    mu = m.param("mu", dim="k")
    D2 = m.data("d2", d2.reshape(-1), dim=kk.name)
    eye = m.data("eye", np.eye(K).reshape(-1), dim=kk.name)
    Y = m.data("y", y.reshape(-1), dim=kn.name)
    C = S.exp(2.0 * log_amp) * S.exp(-0.5 * D2 * S.exp(-2.0 * log_ls)) + S.exp(2.0 * log_noise) * eye
    m.add_logp(S.mvnormal_lpdf(Y, m.broadcast(mu, "k", "obs"), cov=C))
    if factor_deterministic:      # (a reported value built on a matrix stage: the generated expand function runs it too)
        m.deterministic("cov_chol", S.cholesky(C))
    for p in (log_amp, log_ls, log_noise):
        m.add_logp(S.normal_lpdf(p, -0.5, 1.0))
    m.add_logp(S.normal_lpdf(mu, 0.0, 1.0).sum())
    return m


def lkj_prior(K: int = 3, eta: float = 2.0):
    """The LKJ-Cholesky covariance alone (standard deviations HalfNormal(1)): a law test of its correlations"""
    m = S.Model()
    L, sd = m.lkj_cholesky_cov("chol", K, eta, lambda s: S.halfnormal_lpdf(s, 1.0))
    m.deterministic("chol_sd", sd)
    return m, L


def correlated_rows(K: int = 2, N: int = 40, seed: int = 3, rho: float = 0.6):
    """Correlated K-vectors with an LKJ-Cholesky covariance (eta = 2, HalfNormal(1) standard deviations): the data are N draws"""
    rng = np.random.default_rng(seed)
    sd = np.linspace(0.5, 1.5, K)
    R = np.full((K, K), rho) + (1.0 - rho) * np.eye(K)
    y = (np.linalg.cholesky(sd[:, None] * R * sd[None, :]) @ rng.normal(size=(K, N))).reshape(-1)
    m = S.Model()
    L, _ = m.lkj_cholesky_cov("chol", K, 2.0, lambda s: S.halfnormal_lpdf(s, 1.0))
    m.dim("obs", N)
    kn = m.product("chol_k", "obs")
    Y = m.data("y", y, dim=kn.name)
    m.add_logp(S.mvnormal_lpdf(Y, 0.0, chol=L))
    return m

