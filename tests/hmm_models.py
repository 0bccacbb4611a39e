"""The hidden-Markov models the HMM tests share (tests/test_hmm_cpu.py, tests/test_gpu_hmm.py) and tests/prebuild_hmm_cache.py compiles
ahead of time: the regime-switching example of nutpie_amd/timeseries.py, its panel variant, their torch twins."""
import numpy as np

EXAMPLE = dict(T=60, K=2)                 # the example as the GPU tests sample it
PANEL = dict(T=20, K=3, R=5)              # a panel of five series with three states
LAW = dict(T=30, K=2)                     # the comparison of the compiled example with its eager twin


def example(**kw):
    from nutpie_amd.timeseries import regime_switching_model

    return regime_switching_model(**kw)


def twin(**kw):
    from nutpie_amd.timeseries import regime_switching_torch_density

    return regime_switching_torch_density(**kw)


def traced_twin(**kw):
    from nutpie_amd.compiled_pyfunc import from_torch_density

    D, logp = twin(**kw)
    return from_torch_density(D, logp, compile=True)


def points(model, n, seed=0, scale=0.4):
    """``n`` positions around the model's support point"""
    return model.initial_point() + scale * np.random.default_rng(seed).normal(size=(n, model.n_dim))


def hmm_with_cholesky():
    """the example with a multivariate-normal prior on the state means whose covariance has a free amplitude: an HMM stage and a
    Cholesky stage in one density (one wave per chain: the matrix stages ask for it)"""
    from nutpie_amd import symbolic as S

    K = 3
    m = example(T=12, K=K)
    mu = dict(m._det)["mu"]
    m.dim("one", 1)
    log_amp = m.param("log_amp")
    kk = m.product("P_k", "P_k")
    t = np.arange(K, dtype=np.float64)
    base = m.data("prior_cov", (np.exp(-0.5 * (t[:, None] - t[None, :]) ** 2) + 0.5 * np.eye(K)).reshape(-1), dim=kk.name)
    m.add_logp(S.mvnormal_lpdf(m.broadcast(mu, "P_k", "one"), 0.0, cov=S.exp(2.0 * log_amp) * base) + S.normal_lpdf(log_amp, 1.0, 0.5))
    return m
