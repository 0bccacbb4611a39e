"""Linear Gaussian state-space models on the GPU: the compiled local linear trend example and the AR(p) model (nutpie_amd/timeseries.py;
the Kalman stages of csrc/chain_kalman.h inside the generated density) against torch.autograd on their torch twins, at one, two and
four waves per chain; the resident and batched forms; the traced twin; the filtered level from the generated expand function; and
the sampler's law against the same model with its latent path as parameters.  The models: tests/kalman_models.py; DESIGN.md §11.9."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import kalman_models  # noqa: E402

import nutpie_amd  # noqa: E402

pytestmark = pytest.mark.gpu

SCALES = ("sigma_obs_log__", "sigma_level_log__", "sigma_slope_log__", "sigma_seasonal_log__")


def autograd(twin, x):
    import torch

    _, logp = twin
    xt = torch.tensor(x, requires_grad=True)
    lp = logp(xt)
    lp.sum().backward()
    return lp.detach().numpy(), xt.grad.numpy()


@pytest.mark.parametrize("which", ["example", "ar"])
def test_compiled_density_and_gradient_equal_autograd_on_the_twin(hip, which):
    """64 points: log-density and gradient to 1e-12 of the largest element, at W = 1, 2, 4.  The twin is a Python loop over the steps in
    matrix form that torch.autograd differentiates.  The AR(p) model's transition matrix depends on the parameters: its gradient
    rows come through Tbar."""
    if which == "example":
        m, twin = kalman_models.example(**kalman_models.EXAMPLE), kalman_models.twin(**kalman_models.EXAMPLE)
    else:
        m, twin = kalman_models.ar(**kalman_models.AR), kalman_models.ar_twin(**kalman_models.AR)
    x = kalman_models.points(m, 64, seed=5)
    lp0, g0 = autograd(twin, x)
    for W in (1, 2, 4):
        lp, g = m.compile(waves_per_chain=W).logp_and_grad(x)
        print(f"{which} W = {W}: logp {np.abs(lp - lp0).max() / np.abs(lp0).max():.3g}, gradient {np.abs(g - g0).max() / np.abs(g0).max():.3g}")
        assert np.abs(lp - lp0).max() <= 1e-12 * np.abs(lp0).max(), W
        assert np.abs(g - g0).max() <= 1e-12 * np.abs(g0).max(), W


def test_resident_and_batched_forms_draw_the_same(hip):
    m = kalman_models.example(**kalman_models.EXAMPLE)
    kw = dict(chains=64, tune=50, draws=50, seed=5, progress_bar=False, adaptation="diag")
    a = nutpie_amd.sample(m.compile(), **kw)
    b = nutpie_amd.sample(m.compile(resident=False), **kw)
    for name in ("sigma_obs", "sigma_level", "sigma_slope", "sigma_seasonal", "filtered_level"):
        assert np.array_equal(a.posterior[name].values, b.posterior[name].values), name
    assert np.array_equal(a.sample_stats.n_steps.values, b.sample_stats.n_steps.values)


def test_traced_twin_compiles_onto_the_stage(hip):
    shape = kalman_models.EXAMPLE
    traced = kalman_models.traced_twin(**shape)
    assert "nphip_kalman::forward<1, 64, 4, true>(" in traced._source and "nphip_kalman::backward<1, 64, 4, true>(" in traced._source
    sym = kalman_models.example(**shape).compile()
    x = kalman_models.points(kalman_models.example(**shape), 32, seed=9)
    lp_t, g_t = traced.logp_and_grad(x)
    lp_s, g_s = sym.logp_and_grad(x)
    assert np.abs(lp_t - lp_s).max() <= 1e-12 * np.abs(lp_s).max() and np.abs(g_t - g_s).max() <= 1e-12 * np.abs(g_s).max()


def test_filtered_level_from_the_device_expand_equals_numpy(hip):
    m = kalman_models.example(**kalman_models.EXAMPLE)
    c = m.compile()
    assert "nphip_kalman::forward<1, 64, 4, true>(" in c._source.split("nphip_expand")[1]
    tr = nutpie_amd.sample(c, chains=16, tune=60, draws=25, seed=3, progress_bar=False, store_unconstrained=True)
    n = 16 * 25
    u = tr.unconstrained_posterior
    flat = np.concatenate([np.asarray(u[k].values).reshape(n, -1) for k in SCALES], axis=1)
    assert flat.shape == (n, c.n_dim)
    want = np.asarray(c._expand_func(flat, **c._data)["filtered_level"]).reshape(n, -1)
    got = tr.posterior.filtered_level.values.reshape(n, -1)
    assert got.shape == (n, 64)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)


def test_marginal_and_latent_path_forms_sample_the_same_law(hip):
    """A local level model of 40 points in two compiled forms with independent code paths: the level summed out by the Kalman stage
    (m = 1, init_mean = 0, init_cov = 100), and the level as parameters, non-centred, through the scan stage (l0 ~ N(0, 10), level =
    l0 + sigma_level cumsum(z)); the same priors on the two scales.  128 chains, tune 300, draws 200, fixed seeds.  The posterior
    means of the two log scales differ by at most 4 combined standard errors, each run's from its bulk ESS (nutpie_amd.ess);
    neither run has more than 1 % divergent draws.

    How the data, the prior and the target acceptance were chosen — by the divergences of the latent-path run alone, before the
    comparison was looked at (tests/kalman_models.py: LAW_SEED, LAW_PRIOR, LAW_LEVEL_SCALE, LAW_OBS_SCALE).  With HalfNormal(1)
    priors and the sampler's default target acceptance (0.8) the latent-path form diverges in 3 % to 19 % of its draws for every
    data seed 0 .. 7 and every pair of generating scales tried (level 0.1 .. 0.5, observation 0.7 / 1.0): the funnel between
    sigma_level and the path, the geometry the stage exists to remove.  LogNormal(-0.5, 0.5) priors: 5 % to 12 %; LogNormal(-0.5, 0.3):
    5 % to 7 %.  With target_accept = 0.95 (both runs): HalfNormal(1) 0.7 % to 10 %, LogNormal(-0.5, 0.5) 0.4 % to 3 %,
    LogNormal(-0.5, 0.3) 0.2 % to 0.7 % at the seeds 0 .. 3 of either pair of scales.  Taken: LogNormal(-0.5, 0.3), target_accept =
    0.95, data drawn with level scale 0.5 and observation scale 0.7, and the first seed, 0 (0.20 %)."""
    from nutpie_amd.ess import ess_bulk

    kw = dict(chains=128, tune=300, draws=200, target_accept=0.95, progress_bar=False, store_unconstrained=True)
    a = nutpie_amd.sample(kalman_models.local_level_marginal().compile(), seed=11, **kw)
    b = nutpie_amd.sample(kalman_models.local_level_latent().compile(), seed=12, **kw)
    da, db = a.sample_stats.diverging.values.mean(), b.sample_stats.diverging.values.mean()
    print(f"divergent draws: marginal {da:.4f}, latent path {db:.4f}")
    assert da <= 0.01 and db <= 0.01
    for name in SCALES[:2]:
        va = np.asarray(a.unconstrained_posterior[name].values).reshape(kw["chains"], kw["draws"])
        vb = np.asarray(b.unconstrained_posterior[name].values).reshape(kw["chains"], kw["draws"])
        se = np.sqrt(va.var() / ess_bulk(va) + vb.var() / ess_bulk(vb))
        print(f"{name}: marginal {va.mean():.4f}, latent path {vb.mean():.4f}, combined standard error {se:.4f}")
        assert abs(va.mean() - vb.mean()) <= 4.0 * se, (name, va.mean(), vb.mean(), se)
