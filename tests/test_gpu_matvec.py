"""Products with a wide design matrix on the GPU: the generated data-matrix stages (csrc/chain_matvec.h) against the numpy evaluation
at one, two and four waves per chain, in LDS and in device memory; bitwise independence of the waves per chain; the resident, batched
and low-rank forms; chain sharding; the sampler's law against the closed-form posterior of a Gaussian linear regression; the traced
torch twin."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import regression_models as rm  # noqa: E402

import nutpie_amd  # noqa: E402

pytestmark = pytest.mark.gpu

# (n, k): one row; a ragged last block of rows with every lane of one wave owning a column; the flagship shape (k = 200: column blocks
# of a lane partly past the end); n = 20 000: the per-chain arrays on the rows live in device memory
SHAPES = [(1, 33), (65, 64), (2000, 200), (20000, 64)]


@pytest.mark.parametrize("n,k", SHAPES)
@pytest.mark.parametrize("W", [1, 2, 4])
def test_device_products_equal_the_numpy_evaluation(hip, n, k, W):
    c = rm.probe_model(n, k, seed=n + k).compile(waves_per_chain=W)
    if n == 20000:
        assert "data.scratch__" in c._source
    x = rm.points(c.n_dim, 256, seed=n + W)
    lp, g = c.logp_and_grad(x)
    ref = [c.logp_and_grad_numpy(x[i:i + 32]) for i in range(0, len(x), 32)]
    lp_ref, g_ref = np.concatenate([r[0] for r in ref]), np.concatenate([r[1] for r in ref])
    print(f"n={n} k={k} W={W}: max rel logp {np.abs(lp / lp_ref - 1).max():.2e}, max abs grad {np.abs(g - g_ref).max():.2e} "
          f"(max |logp| {np.abs(lp_ref).max():.3e})")
    np.testing.assert_allclose(lp, lp_ref, rtol=1e-11, atol=0)
    np.testing.assert_allclose(g, g_ref, rtol=1e-9, atol=1e-9 * np.abs(lp_ref).max())


@pytest.mark.parametrize("W", [1, 4])
def test_a_narrow_matrix_read_by_the_loops_and_by_a_stage_equals_the_numpy_evaluation(hip, W):
    # 8 columns, stage=None: `X @ beta` is the sum over the columns (its loops read the matrix from the staged copy in LDS), `X.T @ g`
    # and its adjoint are the stage (device memory)
    c = rm.probe_model(50, 8, stage=None).compile(waves_per_chain=W)
    assert "const auto D_X = NPHIP_LDS_CPTR(double" in c._source and "nphip_mv::times_t<8, 1>(data.X, " in c._source
    x = rm.points(c.n_dim, 256, seed=W)
    lp, g = c.logp_and_grad(x)
    lp_ref, g_ref = c.logp_and_grad_numpy(x)
    np.testing.assert_allclose(lp, lp_ref, rtol=1e-11, atol=0)
    np.testing.assert_allclose(g, g_ref, rtol=1e-9, atol=1e-9 * np.abs(lp_ref).max())


def test_a_matrix_with_more_column_blocks_than_a_lane_keeps_side_by_side(hip):
    # 600 columns at one wave per chain: ten column blocks per lane, taken four at a time (chain_matvec.h: COLB)
    c = rm.probe_model(70, 600, seed=9).compile(waves_per_chain=1)
    x = rm.points(c.n_dim, 64, seed=2)
    lp, g = c.logp_and_grad(x)
    lp_ref, g_ref = c.logp_and_grad_numpy(x)
    np.testing.assert_allclose(lp, lp_ref, rtol=1e-11, atol=0)
    np.testing.assert_allclose(g, g_ref, rtol=1e-9, atol=1e-9 * np.abs(lp_ref).max())


@pytest.mark.parametrize("W", [1, 2, 4])
def test_device_products_with_four_right_hand_sides_equal_the_numpy_evaluation(hip, W):
    n, k, R = 2000, 50, 4
    c = rm.probe_model_rhs(n, k, R, seed=n + k).compile(waves_per_chain=W)
    assert "nphip_mv::times<50, 4>" in c._source and "nphip_mv::times_t<50, 4>" in c._source
    x = rm.points(c.n_dim, 256, seed=n + W)
    lp, g = c.logp_and_grad(x)
    ref = [c.logp_and_grad_numpy(x[i:i + 32]) for i in range(0, len(x), 32)]
    lp_ref, g_ref = np.concatenate([r[0] for r in ref]), np.concatenate([r[1] for r in ref])
    print(f"n={n} k={k} R={R} W={W}: max rel logp {np.abs(lp / lp_ref - 1).max():.2e}, max abs grad {np.abs(g - g_ref).max():.2e} "
          f"(max |logp| {np.abs(lp_ref).max():.3e})")
    np.testing.assert_allclose(lp, lp_ref, rtol=1e-11, atol=0)
    np.testing.assert_allclose(g, g_ref, rtol=1e-9, atol=1e-9 * np.abs(lp_ref).max())


def test_the_gradient_of_the_coefficients_does_not_depend_on_the_waves_per_chain(hip):
    # the gradient rows of beta are the transposed product's output plus an element-wise term: bitwise the same at W = 1, 2, 4 (the
    # order contract of chain_matvec.h); logp and the rows of a and sigma go through the W-dependent wave sums
    m = rm.gaussian_model(2000, 200, seed=3)
    x = rm.points(m.n_dim, 256, seed=4)
    out = {W: m.compile(waves_per_chain=W).logp_and_grad(x) for W in (1, 2, 4)}
    off = 2          # [a, sigma_log__, beta (200)]
    for W in (2, 4):
        assert np.array_equal(out[W][1][:, off:], out[1][1][:, off:]), W
        np.testing.assert_allclose(out[W][0], out[1][0], rtol=1e-12)


def test_resident_batched_and_low_rank_forms(hip):
    kw = dict(chains=32, tune=150, draws=60, seed=5, progress_bar=False)
    # (low_rank below the size where the engine's two low-rank forms part during warm-up whatever the density: DESIGN.md §11.6)
    for adapt, k in (("diag", 200), ("low_rank", 100)):
        m = rm.logistic(2000, k)
        a = nutpie_amd.sample(m.compile(), adaptation=adapt, **kw)
        b = nutpie_amd.sample(m.compile(resident=False), adaptation=adapt, **kw)
        assert np.array_equal(a.posterior.beta.values, b.posterior.beta.values), adapt
        assert np.array_equal(a.posterior.a.values, b.posterior.a.values), adapt
        assert np.array_equal(a.sample_stats.n_steps.values, b.sample_stats.n_steps.values), adapt


@pytest.mark.parametrize("W", [1, 4])
def test_chain_sharding_invariance_and_repeatability(hip, W):
    c = rm.logistic(300, 64).compile(waves_per_chain=W)
    kw = dict(tune=100, draws=40, seed=17, progress_bar=False)
    big = nutpie_amd.sample(c, chains=64, **kw)
    small = nutpie_amd.sample(c, chains=8, **kw)
    again = nutpie_amd.sample(c, chains=8, **kw)
    assert np.array_equal(big.posterior.beta.values[:8], small.posterior.beta.values)
    assert np.array_equal(small.posterior.beta.values, again.posterior.beta.values)
    assert np.array_equal(small.posterior.a.values, again.posterior.a.values)


def test_gaussian_linear_regression_draws_follow_the_closed_form_posterior(hip):
    from nutpie_amd.regression import linear_regression_model

    n, k, chains, sigma = 500, 64, 256, 0.5
    X, y = rm.gaussian_data(n, k)
    c = linear_regression_model(X, y, sigma=sigma, prior_sd=1.0).compile()
    assert "nphip_mv::times<64, 1>" in c._source
    # the posterior of [a, beta] in closed form: S = (Z^T Z / sigma^2 + I)^-1, m = S Z^T y / sigma^2 with Z = [1, X]
    Z = np.concatenate([np.ones((n, 1)), X], axis=1)
    cov = np.linalg.inv(Z.T @ Z / sigma ** 2 + np.eye(k + 1))
    mean = cov @ (Z.T @ y) / sigma ** 2
    tr = nutpie_amd.sample(c, chains=chains, tune=400, draws=200, seed=21, progress_bar=False)
    assert not tr.sample_stats.diverging.values.any()
    beta = tr.posterior.beta.values                     # [chains, draws, k]
    m, s = mean[1:], np.diag(cov)[1:]                   # (the vector is [a, beta])
    a_c = beta.mean(1)                                  # chain means: independent estimates of the posterior mean ...
    b_c = ((beta - m) ** 2).mean(1)                     # ... and, the mean being known, unbiased ones of the variance
    z_mean = np.abs(a_c.mean(0) - m) / np.sqrt(a_c.var(0, ddof=1) / chains)
    z_var = np.abs(b_c.mean(0) - s) / np.sqrt(b_c.var(0, ddof=1) / chains)
    print(f"largest |z| of the 64 means {z_mean.max():.2f}, of the 64 variances {z_var.max():.2f}")
    assert (z_mean < 5.0).all(), z_mean
    assert (z_var < 5.0).all(), z_var


def test_the_traced_twin_is_the_symbolic_model(hip):
    from nutpie_amd.regression import logistic_regression_model, logistic_regression_torch_density
    from nutpie_amd.torch_trace import trace

    X, y = rm.logistic_data(2000, 200)
    D, logp = logistic_regression_torch_density(X, y)
    sym = logistic_regression_model(X, y).compile()
    traced = trace(logp, D).compile()
    assert "nphip_mv::times<200, 1>" in traced._source
    x = rm.points(D, 256, seed=6)
    lp_s, g_s = sym.logp_and_grad(x)
    lp_t, g_t = traced.logp_and_grad(x)
    np.testing.assert_allclose(lp_t, lp_s, rtol=1e-11, atol=0)
    np.testing.assert_allclose(g_t, g_s, rtol=1e-9, atol=1e-9 * np.abs(lp_s).max())
    with warnings.catch_warnings():
        warnings.simplefilter("error")                  # (compile="auto" announces a fall-back to the eager path with a warning)
        auto = nutpie_amd.from_torch_density(D, logp, compile="auto")
    assert "nphip_mv::times_t<200, 1>" in auto._source


def test_a_deterministic_downstream_of_the_stages_from_the_device_expand_equals_numpy(hip):
    c = rm.reporting_model(300, 64, report_mu=False).compile()      # (values on fixed-size dimensions only: the expand step is generated code)
    assert "nphip_mv::times_t<64, 1>" in c._source.split("nphip_expand")[1]
    tr = nutpie_amd.sample(c, chains=16, tune=100, draws=30, seed=3, progress_bar=False)
    p = tr.posterior
    n = 16 * 30
    flat = np.concatenate([p.a.values.reshape(n, 1), np.log(p.sigma.values).reshape(n, 1), p.beta.values.reshape(n, -1)], axis=1)
    want = c._expand_func(flat, **c._data)["score"]
    np.testing.assert_allclose(p.score.values.reshape(n, -1), np.asarray(want).reshape(n, -1), rtol=1e-12, atol=1e-12 * np.abs(want).max())
