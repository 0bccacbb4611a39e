"""Per-chain dense matrices on the GPU: the generated cholesky / triangular-solve stages (csrc/chain_linalg.h) against the numpy
evaluation, in the resident, batched and low-rank forms; an LKJ law test; recovery of a correlation and of a GP length-scale."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import matrix_models as mm  # noqa: E402

import nutpie_amd  # noqa: E402

pytestmark = pytest.mark.gpu


def _points(c, n, seed):
    rng = np.random.default_rng(seed)
    K = c.n_dim - 3
    return np.concatenate([rng.normal([-0.2, -0.4, -1.5], 0.2, size=(n, 3)), 0.3 * rng.normal(size=(n, K))], axis=1)


@pytest.mark.parametrize("K", [1, 2, 3, 8, 32])
@pytest.mark.parametrize("N", [1, 85])
def test_generated_matrix_stages_equal_the_numpy_evaluation(hip, K, N):
    c = mm.gp_rows(K, N).compile()
    x = _points(c, 256, K * 1000 + N)
    lp, g = c.logp_and_grad(x)
    lp_ref, g_ref = c.logp_and_grad_numpy(x)
    np.testing.assert_allclose(lp, lp_ref, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(g, g_ref, rtol=1e-8, atol=1e-8 * np.abs(lp_ref).max())


def test_a_point_that_is_not_positive_definite_is_nonfinite_on_the_device(hip):
    from nutpie_amd import symbolic as S

    m = S.Model()
    m.dim("k", 2)
    kk = m.product("k", "k")
    r = m.param("r")
    A = m.data("one", np.array([1.0, 0.0, 0.0, 1.0]), dim=kk.name) + r * m.data("off", np.array([0.0, 1.0, 1.0, 0.0]), dim=kk.name)
    m.add_logp(S.log_det_chol(S.cholesky(A)) - 0.5 * r * r)
    c = m.compile()
    lp, _ = c.logp_and_grad(np.array([[0.5], [2.0], [-1.0], [0.0]]))
    assert np.isfinite(lp[0]) and np.isfinite(lp[3]) and not np.isfinite(lp[1]) and not np.isfinite(lp[2])


def test_resident_batched_and_low_rank_forms(hip):
    m = mm.gp_rows(3, 85)
    kw = dict(chains=32, tune=150, draws=60, seed=5, progress_bar=False)
    a = nutpie_amd.sample(m.compile(), **kw)
    b = nutpie_amd.sample(m.compile(resident=False), **kw)
    assert np.array_equal(a.posterior.mu.values, b.posterior.mu.values)
    assert np.array_equal(a.sample_stats.n_steps.values, b.sample_stats.n_steps.values)
    # the low-rank leaf: the same comparison under adaptation="low_rank"
    lr = nutpie_amd.sample(m.compile(), adaptation="low_rank", **kw)
    lrb = nutpie_amd.sample(m.compile(resident=False), adaptation="low_rank", **kw)
    assert np.array_equal(lr.posterior.mu.values, lrb.posterior.mu.values)
    assert np.array_equal(lr.sample_stats.n_steps.values, lrb.sample_stats.n_steps.values)
    assert np.all(np.isfinite(lr.posterior.log_ls.values))
    assert abs(lr.posterior.log_ls.values.mean() - a.posterior.log_ls.values.mean()) < 0.3


def test_a_deterministic_on_a_matrix_stage_from_the_device_expand(hip):
    c = mm.gp_rows(4, 6, factor_deterministic=True).compile()
    tr = nutpie_amd.sample(c, chains=16, tune=100, draws=30, seed=3, progress_bar=False)
    want = c._expand_func(_flat(tr), **c._data)["cov_chol"]       # the numpy evaluation of the same draws
    np.testing.assert_allclose(tr.posterior.cov_chol.values.reshape(16 * 30, -1), np.asarray(want).reshape(16 * 30, -1), rtol=1e-12, atol=1e-14)


def _flat(tr):
    p = tr.posterior
    n = p.log_amp.values.size
    return np.concatenate([p.log_amp.values.reshape(n, 1), p.log_ls.values.reshape(n, 1), p.log_noise.values.reshape(n, 1),
                           p.mu.values.reshape(n, -1)], axis=1)


def test_correlated_radon_compiled_and_eager_agree(hip):
    from nutpie_amd.compiled_pyfunc import autograd_logp, from_torchfunc
    from nutpie_amd.radon import correlated_radon_model, correlated_radon_torch_density, synthetic_correlated_radon_data

    data = synthetic_correlated_radon_data()
    kw = dict(chains=128, tune=400, draws=200, progress_bar=False)
    comp = nutpie_amd.sample(correlated_radon_model(data).compile(), seed=11, **kw)
    assert comp.sample_stats.diverging.values.sum() == 0
    corr = comp.posterior.chol_corr.values.reshape(-1)
    lo, hi = np.quantile(corr, [0.005, 0.995])
    assert lo < data["rho"] < hi
    D, logp = correlated_radon_torch_density(data, device="cuda")
    eager = nutpie_amd.sample(from_torchfunc(D, lambda: autograd_logp(logp)), seed=12, **kw)
    x_c = np.concatenate([comp.posterior[n].values.reshape(128, 200, -1) for n in ("intercept", "floor_effect")], axis=2)
    x_c = np.concatenate([x_c, np.log(comp.posterior.sigma.values)[..., None]], axis=2)
    x_e = eager.posterior.x.values[..., :3]
    for k in range(3):   # intercept, floor effect, log sigma: chain means as independent estimates of the posterior mean
        ma, mb = x_c[..., k].mean(1), x_e[..., k].mean(1)
        se = np.sqrt(ma.var() / ma.size + mb.var() / mb.size)
        assert abs(ma.mean() - mb.mean()) < 5 * se, k


def test_chain_sharding_invariance(hip):
    c = mm.gp_rows(8, 20).compile()
    kw = dict(tune=100, draws=40, seed=17, progress_bar=False)
    big = nutpie_amd.sample(c, chains=64, **kw)
    small = nutpie_amd.sample(c, chains=8, **kw)
    assert np.array_equal(big.posterior.mu.values[:8], small.posterior.mu.values)
    assert np.array_equal(big.posterior.log_amp.values[:8], small.posterior.log_amp.values)


def test_lkj_prior_correlations_follow_their_beta_law(hip):
    from scipy import stats

    K, eta = 3, 2.0
    m, _ = mm.lkj_prior(K, eta)
    tr = nutpie_amd.sample(m.compile(), chains=256, tune=400, draws=200, seed=8, progress_bar=False)
    packed = tr.posterior["chol_cholesky-cov-packed__"].values.reshape(-1, K * (K + 1) // 2)
    L = np.zeros((packed.shape[0], K, K))
    rows, cols = np.tril_indices(K)
    L[:, rows, cols] = packed
    d = np.arange(K)
    L[:, d, d] = np.exp(L[:, d, d])
    C = L / np.sqrt((L**2).sum(axis=2, keepdims=True))
    R = C @ np.transpose(C, (0, 2, 1))
    a = eta - 1.0 + K / 2.0
    law = stats.beta(a, a, loc=-1.0, scale=2.0)          # 2 Beta(a, a) - 1
    for i, j in ((1, 0), (2, 0), (2, 1)):
        r = R[:, i, j]
        assert abs(r.mean()) < 0.02
        assert abs(r.var() / law.var() - 1.0) < 0.06
        assert stats.kstest(r, law.cdf).statistic < 0.02
    # (the prior alone puts standard deviations near zero, a funnel: a rare divergence there is the geometry's, not the density's)
    assert tr.sample_stats.diverging.values.mean() < 1e-3


def test_correlated_rows_recover_their_correlation(hip):
    rho = 0.6
    m = mm.correlated_rows(K=2, N=80, rho=rho)
    tr = nutpie_amd.sample(m.compile(), chains=64, tune=400, draws=200, seed=21, progress_bar=False)
    assert tr.sample_stats.diverging.values.sum() == 0
    p = tr.posterior["chol_cholesky-cov-packed__"].values.reshape(-1, 3)
    r = p[:, 1] / np.sqrt(p[:, 1] ** 2 + np.exp(2 * p[:, 2]))     # L[1][0] / |row 1|
    lo, hi = np.quantile(r, [0.005, 0.995])
    assert lo < rho < hi


def test_traced_gp_marginal_likelihood_samples_and_covers_its_length_scale(hip):
    import torch
    from torch.distributions import MultivariateNormal

    # (n = 30 points: one chain's matrix is at most 32 x 32)
    n2, ls, amp, noise = 30, 0.8, 1.0, 0.2
    rng = np.random.default_rng(2)
    t = np.sort(rng.uniform(0, 6, n2))
    K_ = amp**2 * np.exp(-0.5 * (t[:, None] - t[None, :]) ** 2 / ls**2) + noise**2 * np.eye(n2)
    y2 = torch.as_tensor(np.linalg.cholesky(K_) @ rng.normal(size=n2))
    d22 = torch.as_tensor((t[:, None] - t[None, :]) ** 2)
    eye2 = torch.eye(n2, dtype=torch.float64)

    def logp2(x):
        C = torch.exp(2 * x[0, 0]) * torch.exp(-0.5 * d22 * torch.exp(-2 * x[0, 1])) + torch.exp(2 * x[0, 2]) * eye2
        return (MultivariateNormal(torch.zeros(n2, dtype=torch.float64), covariance_matrix=C).log_prob(y2) - 0.5 * (x * x).sum()).reshape(1)

    model = nutpie_amd.from_torch_density(3, logp2, compile=True)
    tr = nutpie_amd.sample(model, chains=64, tune=400, draws=200, seed=4, progress_bar=False)
    lls = np.exp(tr.posterior.x.values[..., 1]).reshape(-1)
    lo, hi = np.quantile(lls, [0.005, 0.995])
    assert lo < ls < hi
