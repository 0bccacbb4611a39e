"""The state-space models the Kalman tests share (tests/test_kalman_cpu.py, tests/test_gpu_kalman.py) and tests/prebuild_kalman_cache.py
compiles ahead of time: the local linear trend example of nutpie_amd/timeseries.py, its panel variant, the AR(p) model, their torch
twins, and the two forms of the local level model of the law test."""
import numpy as np

EXAMPLE = dict(T=64, seasonal_period=12)          # the example as the GPU tests evaluate it: level + slope + one harmonic, m = 4
PANEL = dict(T=20, R=5)                           # a panel of five series, m = 2
AR = dict(T=64, p=3)                              # AR(3) in companion form: the transition depends on the parameters
LAW_T = 40
LAW_SEED = 0                                      # the data seed of the law test (see tests/test_gpu_kalman.py)
LAW_LEVEL_SCALE, LAW_OBS_SCALE = 0.5, 0.7         # the scales the law test's data are drawn with
LAW_PRIOR = (-0.5, 0.3)                           # the prior of the two scales: None = HalfNormal(1), (mu, sd) = LogNormal


def example(**kw):
    from nutpie_amd.timeseries import local_linear_trend_model

    return local_linear_trend_model(**kw)


def twin(**kw):
    """the independent implementation: a Python loop over the steps with torch.autograd"""
    from nutpie_amd.timeseries import local_linear_trend_torch_density

    return local_linear_trend_torch_density(**kw)


def op_twin(**kw):
    """the same density with the custom op torch_trace.kalman_marginal"""
    from nutpie_amd.timeseries import local_linear_trend_op_density

    return local_linear_trend_op_density(**kw)


def traced_twin(**kw):
    from nutpie_amd.compiled_pyfunc import from_torch_density

    D, logp = op_twin(**kw)
    return from_torch_density(D, logp, compile=True)


def ar(**kw):
    from nutpie_amd.timeseries import ar_p_model

    return ar_p_model(**kw)


def ar_twin(**kw):
    from nutpie_amd.timeseries import ar_p_torch_density

    return ar_p_torch_density(**kw)


def points(model, n, seed=0, scale=0.4):
    """``n`` positions around the model's support point"""
    return model.initial_point() + scale * np.random.default_rng(seed).normal(size=(n, model.n_dim))


def kalman_with_cholesky():
    """the AR model with a multivariate-normal prior on rho whose covariance has a free amplitude: a Kalman stage and a Cholesky stage
    in one density (one wave per chain: the matrix stages ask for it)"""
    from nutpie_amd import symbolic as S

    p = 3
    m = ar(T=12, p=p)
    rho = next(q for q in m._params if q.dim is not None)
    m.dim("one", 1)
    log_amp = m.param("log_amp")
    t = np.arange(p, dtype=np.float64)
    base = m.data("prior_cov", (np.exp(-0.5 * (t[:, None] - t[None, :]) ** 2) + 0.5 * np.eye(p)).reshape(-1), dim=m.product("state", "state").name)
    m.add_logp(S.mvnormal_lpdf(m.broadcast(rho, "state", "one"), 0.0, cov=S.exp(2.0 * log_amp) * base) + S.normal_lpdf(log_amp, 1.0, 0.5))
    return m


# --------------------------------------------------------------------------- the law test's two forms of one model
def local_level_data(T=LAW_T, seed=LAW_SEED, level_scale=LAW_LEVEL_SCALE, obs_scale=LAW_OBS_SCALE):
    rng = np.random.default_rng(1000 + seed)
    return 1.0 + np.cumsum(level_scale * rng.normal(size=T)) + obs_scale * rng.normal(size=T)


def _scales(m, prior=None):
    """the two positive scales with the prior both forms share: HalfNormal(1), or (``prior`` = (mu, sd)) LogNormal(mu, sd)"""
    from nutpie_amd import symbolic as S

    s_obs, s_level = m.param("sigma_obs", lower=0.0), m.param("sigma_level", lower=0.0)
    for s in (s_obs, s_level):
        m.add_logp(S.halfnormal_lpdf(s, 1.0) if prior is None else S.normal_lpdf(S.log(s), prior[0], prior[1]) - S.log(s))
    return s_obs, s_level


def local_level_marginal(T=LAW_T, seed=LAW_SEED, prior=LAW_PRIOR, **data):
    """both scales ~ LogNormal(-0.5, 0.3) (``prior``); level_0 ~ N(0, 10^2), level_{t+1} = level_t + sigma_level e, y_t = level_t + sigma_obs e with the level summed out: the Kalman
    stage with m = 1, init_mean = 0, init_cov = 100.  Vector: [sigma_obs_log__, sigma_level_log__]."""
    from nutpie_amd import symbolic as S

    m = S.Model()
    s_obs, s_level = _scales(m, prior)
    m.dim("time", T)
    m.dim("state", 1)
    one = m.product("state", "state")
    y = m.data("y", local_level_data(T, seed, **data), dim="time")
    m.add_logp(S.kalman_marginal_lpdf(y, design=m.data("design", np.ones(1), dim="state"), obs_var=s_obs * s_obs,
                                      transition=m.data("transition", np.ones(1), dim=one.name), state_cov=S.stack([s_level * s_level], one),
                                      init_mean=0.0, init_cov=m.data("init_cov", np.full(1, 100.0), dim=one.name)))
    return m


def local_level_latent(T=LAW_T, seed=LAW_SEED, prior=LAW_PRIOR, **data):
    """the same model with its path as parameters, non-centred: level = l0 + sigma_level cumsum(z) through the scan stage, l0 ~ N(0, 10),
    z_0 = 0 by construction (z holds the T - 1 increments).  Vector: [sigma_obs_log__, sigma_level_log__, l0, z (T)]; z_0 is a
    standard normal that the likelihood does not see."""
    from nutpie_amd import symbolic as S

    m = S.Model()
    s_obs, s_level = _scales(m, prior)
    m.dim("time", T)
    l0 = m.param("l0")
    z = m.param("z", dim="time")
    first = np.zeros(T)
    first[0] = 1.0
    keep = m.data("after_first", 1.0 - first, dim="time")
    m.add_logp(S.normal_lpdf(l0, 0.0, 10.0) + S.normal_lpdf(z, 0.0, 1.0).sum())
    level = l0 + s_level * S.cumsum(keep * z)
    m.add_logp(S.normal_lpdf(m.data("y", local_level_data(T, seed, **data), dim="time"), level, s_obs).sum())
    return m
