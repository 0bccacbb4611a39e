"""Hidden Markov models on the GPU: the compiled regime-switching example (nutpie_amd/timeseries.py; the HMM stages of
csrc/chain_hmm.h inside the generated density) against torch.autograd on its torch twin, at one, two and four waves per chain; the
resident and batched forms; the traced twin; the smoothed state probabilities from the generated expand function; and the sampler's
law against the eager torch twin.  The models: tests/hmm_models.py; DESIGN.md §11.8."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import hmm_models  # noqa: E402

import nutpie_amd  # noqa: E402

pytestmark = pytest.mark.gpu


def autograd_on_the_twin(shape, x):
    import torch

    _, logp = hmm_models.twin(**shape)
    xt = torch.tensor(x, requires_grad=True)
    lp = logp(xt)
    lp.sum().backward()
    return lp.detach().numpy(), xt.grad.numpy()


@pytest.mark.parametrize("shape", [hmm_models.EXAMPLE, hmm_models.PANEL], ids=["example", "panel"])
def test_compiled_density_and_gradient_equal_autograd_on_the_twin(hip, shape):
    """64 points: log-density and gradient to 1e-12 of the largest element.  At W = 1, 2, 4 the gradient rows of the vector
    parameters (the state means and the rows of the transition matrix: the stages' outputs through segment sums of fixed order)
    have the same bits; logp and the row of the scalar sigma go through the W-dependent wave sums of the generated loops, as for the
    other stages (tests/test_gpu_matvec.py)."""
    m = hmm_models.example(**shape)
    x = hmm_models.points(m, 64, seed=5)
    lp0, g0 = autograd_on_the_twin(shape, x)
    out = {W: m.compile(waves_per_chain=W).logp_and_grad(x) for W in (1, 2, 4)}
    K = shape["K"]
    vector_rows = [i for i in range(m.n_dim) if i != K]        # [mu (K), sigma_log__, the K rows of P (K - 1 each)]
    for W, (lp, g) in out.items():
        assert np.abs(lp - lp0).max() <= 1e-12 * np.abs(lp0).max(), W
        assert np.abs(g - g0).max() <= 1e-12 * np.abs(g0).max(), W
        print(f"W = {W}: all gradient rows equal to W = 1: {np.array_equal(g, out[1][1])}, logp: {np.array_equal(lp, out[1][0])}")
        assert np.array_equal(g[:, vector_rows], out[1][1][:, vector_rows]), W


def test_resident_and_batched_forms_draw_the_same(hip):
    m = hmm_models.example(**hmm_models.EXAMPLE)
    kw = dict(chains=64, tune=50, draws=50, seed=5, progress_bar=False, adaptation="diag")
    a = nutpie_amd.sample(m.compile(), **kw)
    b = nutpie_amd.sample(m.compile(resident=False), **kw)
    for name in ("mu", "sigma", "P", "state_prob"):
        assert np.array_equal(a.posterior[name].values, b.posterior[name].values), name
    assert np.array_equal(a.sample_stats.n_steps.values, b.sample_stats.n_steps.values)


def test_traced_twin_samples(hip):
    D, logp = hmm_models.twin(**hmm_models.EXAMPLE)
    traced = hmm_models.traced_twin(**hmm_models.EXAMPLE)
    assert "nphip_hmm::forward<1, 60, 2>(" in traced._source
    eager = nutpie_amd.from_torch_density(D, logp, compile=False)
    tr = nutpie_amd.sample(traced, chains=16, tune=60, draws=20, seed=2, progress_bar=False)
    assert list(tr.posterior.data_vars) == list(eager._names) == ["x"] and tr.posterior.x.shape == (16, 20, D)
    # the same flat vector as the symbolic example: the two device densities at the same points
    sym = hmm_models.example(**hmm_models.EXAMPLE).compile()
    x = hmm_models.points(hmm_models.example(**hmm_models.EXAMPLE), 32, seed=9)
    lp_t, g_t = traced.logp_and_grad(x)
    lp_s, g_s = sym.logp_and_grad(x)
    assert np.abs(lp_t - lp_s).max() <= 1e-12 * np.abs(lp_s).max() and np.abs(g_t - g_s).max() <= 1e-12 * np.abs(g_s).max()


def test_smoothed_probabilities_from_the_device_expand_equal_numpy(hip):
    m = hmm_models.example(**hmm_models.EXAMPLE)
    c = m.compile()
    assert "nphip_hmm::backward<1, 60, 2>(" in c._source.split("nphip_expand")[1]
    tr = nutpie_amd.sample(c, chains=16, tune=60, draws=25, seed=3, progress_bar=False, store_unconstrained=True)
    n = 16 * 25
    u = tr.unconstrained_posterior       # the flat vector: [mu_ordered__ (2), sigma_log__, P_0_simplex__ (1), P_1_simplex__ (1)]
    flat = np.concatenate([np.asarray(u[k].values).reshape(n, -1) for k in ("mu_ordered__", "sigma_log__", "P_0_simplex__", "P_1_simplex__")], axis=1)
    assert flat.shape == (n, c.n_dim)
    want = np.asarray(c._expand_func(flat, **c._data)["state_prob"]).reshape(n, -1)
    got = tr.posterior.state_prob.values.reshape(n, -1)
    assert got.shape == (n, 60 * 2) and np.abs(got.reshape(n, 60, 2).sum(-1) - 1.0).max() <= 1e-14
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)


def test_compiled_example_and_eager_twin_sample_the_same_law(hip):
    """T = 30, tune 150, draws 100, fixed seeds; the compiled example against its EAGER torch twin (an independent implementation: a
    Python loop over t in log space with torch.autograd — the only way to run this model without the stage).  For every free
    parameter — its constrained value: the K means, sigma, the K - 1 free entries of every row of P — the posterior means differ
    by at most 4 standard errors, each run's from its bulk ESS (nutpie_amd.ess), combined in quadrature; neither run has more than
    1 % divergent draws."""
    from nutpie_amd.ess import ess_bulk

    shape = hmm_models.LAW
    K = shape["K"]
    m = hmm_models.example(**shape)
    c = m.compile()
    D, logp = hmm_models.twin(**shape, device="cuda")
    eager = nutpie_amd.from_torch_density(D, logp, compile=False)
    kw = dict(chains=128, tune=150, draws=100, progress_bar=False)
    a = nutpie_amd.sample(c, seed=11, **kw)
    t0 = time.perf_counter()
    b = nutpie_amd.sample(eager, seed=12, **kw)
    print(f"eager leg: {time.perf_counter() - t0:.1f} s")
    assert a.sample_stats.diverging.values.mean() <= 0.01 and b.sample_stats.diverging.values.mean() <= 0.01
    xb = b.posterior.x.values
    vals_b = c._expand_func(xb.reshape(-1, D), **c._data)
    names = ["mu", "sigma"] + [f"P_{i}" for i in range(K)]
    for name in names:
        va = np.asarray(a.posterior[name].values).reshape(kw["chains"], kw["draws"], -1)
        vb = np.asarray(vals_b[name]).reshape(kw["chains"], kw["draws"], -1)
        for j in range(va.shape[-1] - (1 if name.startswith("P_") else 0)):       # (the last entry of a row is one minus the others)
            se = np.sqrt(va[..., j].var() / ess_bulk(va[..., j]) + vb[..., j].var() / ess_bulk(vb[..., j]))
            assert abs(va[..., j].mean() - vb[..., j].mean()) <= 4.0 * se, (name, j, va[..., j].mean(), vb[..., j].mean(), se)
