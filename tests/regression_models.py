"""Models with a wide design matrix (the data-matrix stages of symbolic.Matrix: `X @ beta`, `X.T @ g`) for the CPU and GPU tests."""
import numpy as np

from nutpie_amd import symbolic as S


def design(n: int, k: int, seed: int = 0) -> np.ndarray:
    return np.random.default_rng(seed).normal(size=(n, k)) / np.sqrt(k)


def probe_model(n: int, k: int, seed: int = 0, stage=True):
    """beta on the k columns, a scalar s.  eta = X beta feeds y ~ N(eta, 0.7); separately c = X^T g with the computed
    g = tanh(w s) (w data on the rows) feeds N(c | 0.1, 1.3): both stages as the user's, both as the other's adjoint."""
    rng = np.random.default_rng(seed + 1)
    m = S.Model()
    beta = m.param("beta", dim="coef", size=k)
    s = m.param("s")
    X = m.matrix("X", design(n, k, seed), dim="obs", cols="coef", stage=stage)
    y = m.data("y", rng.normal(size=n), dim="obs")
    w = m.data("w", rng.normal(size=n), dim="obs")
    m.add_logp(S.normal_lpdf(beta, 0.0, 1.0).sum() + S.normal_lpdf(s, 0.0, 1.0))
    m.add_logp(S.normal_lpdf(y, X @ beta, 0.7).sum())
    m.add_logp(S.normal_lpdf(X.T @ S.tanh(w * s), 0.1, 1.3).sum())
    return m


def gaussian_model(n: int, k: int, seed: int = 0, stage=None):
    """y ~ Normal(a + X beta, sigma), beta ~ Normal(0, 1), a ~ Normal(0, 1), sigma ~ HalfNormal(1)"""
    rng = np.random.default_rng(seed + 2)
    m = S.Model()
    a = m.param("a")
    sigma = m.param("sigma", lower=0.0)
    beta = m.param("beta", dim="coef", size=k)
    X = m.matrix("X", design(n, k, seed), dim="obs", cols="coef", stage=stage)
    y = m.data("y", rng.normal(size=n), dim="obs")
    m.add_logp(S.normal_lpdf(a, 0.0, 1.0) + S.halfnormal_lpdf(sigma, 1.0) + S.normal_lpdf(beta, 0.0, 1.0).sum())
    m.add_logp(S.normal_lpdf(y, a + X @ beta, sigma).sum())
    return m


def logistic(n: int, k: int, seed: int = 0, stage=None):
    from nutpie_amd.regression import logistic_regression_model

    X, y = logistic_data(n, k, seed)
    return logistic_regression_model(X, y, stage=stage)


def logistic_data(n: int, k: int, seed: int = 0):
    from nutpie_amd.regression import synthetic_binary, synthetic_design

    X, eta = synthetic_design(n, k, seed=seed + 11)
    return X, synthetic_binary(eta, seed=seed + 12)


def gaussian_data(n: int, k: int, seed: int = 0):
    from nutpie_amd.regression import synthetic_design, synthetic_response

    X, eta = synthetic_design(n, k, seed=seed + 21)
    return X, synthetic_response(eta, seed=seed + 22)


def points(n_dim: int, n: int, seed: int, scale: float = 0.3) -> np.ndarray:
    return scale * np.random.default_rng(seed).normal(size=(n, n_dim))


def probe_model_rhs(n: int, k: int, R: int, seed: int = 0):
    """the probe with R right-hand sides: B on product(coef, rhs); E = X B feeds y ~ N(E, 0.7) on the n x R values; separately
    C = X^T G with the computed G (column r: tanh(w (s + r / 4))) feeds N(C | 0.1, 1.3)"""
    rng = np.random.default_rng(seed + 1)
    m = S.Model()
    m.dim("coef", k)
    m.dim("rhs", R)
    B = m.param("B", dims=("coef", "rhs"))
    s = m.param("s")
    X = m.matrix("X", design(n, k, seed), dim="obs", cols="coef")
    E = X @ B
    y = m.data("y", rng.normal(size=n * R), dim=E.dim.name)
    w = m.data("w", rng.normal(size=n), dim="obs")
    m.add_logp(S.normal_lpdf(B, 0.0, 1.0).sum() + S.normal_lpdf(s, 0.0, 1.0))
    m.add_logp(S.normal_lpdf(y, E, 0.7).sum())
    G = S.pack_columns([S.tanh(w * (s + 0.25 * r)) for r in range(R)], E.dim)
    m.add_logp(S.normal_lpdf(X.T @ G, 0.1, 1.3).sum())
    return m


def softmax_data(n: int, k: int, R: int, seed: int = 0):
    from nutpie_amd.regression import synthetic_classes, synthetic_design

    X, _ = synthetic_design(n, k, seed=seed + 31)
    return X, synthetic_classes(X, R, seed=seed + 32)


def reporting_model(n: int, k: int, seed: int = 0, report_mu: bool = True):
    """the Gaussian regression of gaussian_model (stage forced) reporting score = X^T (y - mu) (on the coefficients, downstream of both
    stages: generated expand code) and, with report_mu, mu = a + X beta (on the observations: the numpy expand)"""
    rng = np.random.default_rng(seed + 2)
    m = S.Model()
    a = m.param("a")
    sigma = m.param("sigma", lower=0.0)
    beta = m.param("beta", dim="coef", size=k)
    X = m.matrix("X", design(n, k, seed), dim="obs", cols="coef", stage=True)
    y = m.data("y", rng.normal(size=n), dim="obs")
    mu = a + X @ beta
    m.add_logp(S.normal_lpdf(a, 0.0, 1.0) + S.halfnormal_lpdf(sigma, 1.0) + S.normal_lpdf(beta, 0.0, 1.0).sum())
    m.add_logp(S.normal_lpdf(y, mu, sigma).sum())
    if report_mu:
        m.deterministic("mu", mu)
    m.deterministic("score", X.T @ (y - mu))
    return m
