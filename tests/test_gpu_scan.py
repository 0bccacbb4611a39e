"""First-order linear recurrences on the GPU: the generated scan stages (csrc/chain_scan.h) against the numpy evaluation at one, two
and four waves per chain, in LDS and in device memory; the resident, batched and low-rank forms; the time-series examples."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import scan_models as sm  # noqa: E402

import nutpie_amd  # noqa: E402

pytestmark = pytest.mark.gpu

# (T, a, init); T >= 20 000 puts the arrays in device memory.  Up to R T = 2000 the steps' innovations z are parameters, beyond they are data
# (a compiled density with several waves per chain has a few thousand coordinates at most) — so a per-element a (one parameter per
# element) is tested up to R T = 2000.
CASES = [(1, "vector", "param"), (65, "scalar", "param"), (65, "vector", "param"), (2000, "one", "const"), (2000, "vector", "const"),
         (20000, "one", "const"), (100003, "scalar", "param")]
# (R = 8 rows up to T = 20 000)
PARAMS = [(R, T, a, i, W) for R in (1, 8) for T, a, i in CASES for W in (1, 2, 4) if R * T <= 200_000 and (a != "vector" or R * T <= 2000)]


@pytest.mark.parametrize("R,T,a_kind,init_kind,W", PARAMS)
def test_device_scan_equals_the_numpy_evaluation(hip, R, T, a_kind, init_kind, W):
    if R > 1 and init_kind == "param":
        init_kind = "row"
    c = sm.scan_model(R, T, a_kind, init_kind, seed=T, latent=R * T <= 2000).compile(waves_per_chain=W)
    x = sm.points(c.n_dim, 256, seed=R * T + W)
    lp, g = c.logp_and_grad(x)
    # (the numpy checker in blocks of 32 points: its arrays for 256 points of a 100 000-element series would take several GB)
    ref = [c.logp_and_grad_numpy(x[k:k + 32]) for k in range(0, len(x), 32)]
    lp_ref, g_ref = np.concatenate([r[0] for r in ref]), np.concatenate([r[1] for r in ref])
    np.testing.assert_allclose(lp, lp_ref, rtol=1e-11, atol=0)
    np.testing.assert_allclose(g, g_ref, rtol=1e-9, atol=1e-9 * np.abs(lp_ref).max())


def _sv(T=300):
    from nutpie_amd.timeseries import stochastic_volatility_model, synthetic_returns

    return stochastic_volatility_model(synthetic_returns(T))


def test_resident_batched_and_low_rank_forms(hip):
    # T = 200 (D = 203).  At T = 300 (D = 303) the low-rank forms part during warm-up for the same density written WITHOUT a scan
    # (h = mu + L sigma z with L a data matrix of ones below the diagonal) as much as with it: an engine matter, DESIGN.md §11.6
    m = _sv(200)
    kw = dict(chains=32, tune=150, draws=60, seed=5, progress_bar=False)
    for adapt in ("diag", "low_rank"):
        a = nutpie_amd.sample(m.compile(), adaptation=adapt, **kw)
        b = nutpie_amd.sample(m.compile(resident=False), adaptation=adapt, **kw)
        assert np.array_equal(a.posterior.z.values, b.posterior.z.values), adapt
        assert np.array_equal(a.posterior.mu.values, b.posterior.mu.values), adapt
        assert np.array_equal(a.sample_stats.n_steps.values, b.sample_stats.n_steps.values), adapt


@pytest.mark.parametrize("W", [1, 4])
def test_chain_sharding_invariance_and_repeatability(hip, W):
    c = sm.scan_model(8, 100, "vector", "row").compile(waves_per_chain=W)
    kw = dict(tune=100, draws=40, seed=17, progress_bar=False)
    big = nutpie_amd.sample(c, chains=64, **kw)
    small = nutpie_amd.sample(c, chains=8, **kw)
    again = nutpie_amd.sample(c, chains=8, **kw)
    assert np.array_equal(big.posterior.z.values[:8], small.posterior.z.values)
    assert np.array_equal(small.posterior.z.values, again.posterior.z.values)
    assert np.array_equal(small.posterior.x0r.values, again.posterior.x0r.values)


def test_garch11_posterior_covers_the_true_parameters(hip):
    from nutpie_amd.timeseries import garch11_model, synthetic_garch

    tr = nutpie_amd.sample(garch11_model(synthetic_garch(1000)).compile(), chains=64, tune=400, draws=200, seed=3, progress_bar=False)
    assert tr.sample_stats.diverging.values.mean() < 0.01
    for name, true in (("alpha", 0.2), ("beta", 0.7)):
        lo, hi = np.quantile(tr.posterior[name].values.reshape(-1), [0.005, 0.995])
        assert lo < true < hi, (name, lo, hi)


def test_stochastic_volatility_compiled_traced_and_eager_agree(hip):
    from nutpie_amd.compiled_pyfunc import autograd_logp, from_torchfunc
    from nutpie_amd.timeseries import stochastic_volatility_torch_density, synthetic_returns
    from nutpie_amd.torch_trace import trace

    T = 300
    y = synthetic_returns(T)
    D, logp = stochastic_volatility_torch_density(y)
    comp_model = _sv(T).compile()
    traced_model = trace(logp, D).compile()
    assert "nphip_scan::linear_recurrence<1, 300, nphip_scan::A_ONE" in traced_model._source
    # the same flat vector, the same density up to rounding: the first draws of one seed (warm-up included) ...
    short = dict(chains=8, tune=50, draws=5, seed=2, progress_bar=False)
    a = nutpie_amd.sample(comp_model, **short)
    b = nutpie_amd.sample(traced_model, **short)
    np.testing.assert_allclose(b.warmup_posterior.x.values[:, :3, 0], a.warmup_posterior.mu.values[:, :3], rtol=0, atol=1e-6)
    # ... and the two device densities at the same points
    x = sm.points(D, 64, seed=9, scale=0.2)
    x[:, 0] -= 9.0
    lp_c, g_c = comp_model.logp_and_grad(x)
    lp_t, g_t = traced_model.logp_and_grad(x)
    np.testing.assert_allclose(lp_t, lp_c, rtol=1e-10)
    np.testing.assert_allclose(g_t, g_c, rtol=1e-6, atol=1e-6 * np.abs(g_c).max())
    kw = dict(chains=64, tune=400, draws=200, progress_bar=False)
    comp = nutpie_amd.sample(comp_model, seed=11, **kw)
    tr = nutpie_amd.sample(traced_model, seed=12, **kw)
    _, logp_dev = stochastic_volatility_torch_density(y, device="cuda")
    eager = nutpie_amd.sample(from_torchfunc(D, lambda: autograd_logp(logp_dev)), seed=13, **kw)
    est = {"compiled": np.stack([comp.posterior.mu.values, np.log(comp.posterior.sigma.values)], -1),
           "traced": tr.posterior.x.values[..., :2], "eager": eager.posterior.x.values[..., :2]}
    for k in range(2):   # mu, log sigma: chain means as independent estimates of the posterior mean
        ref = est["compiled"][..., k].mean(1)
        for name in ("traced", "eager"):
            other = est[name][..., k].mean(1)
            se = np.sqrt(ref.var() / ref.size + other.var() / other.size)
            assert abs(ref.mean() - other.mean()) < 5 * se, (name, k)


def test_volatility_from_the_device_expand_equals_numpy(hip):
    c = _sv(200).compile()
    tr = nutpie_amd.sample(c, chains=16, tune=100, draws=30, seed=3, progress_bar=False)
    p = tr.posterior
    n = 16 * 30
    flat = np.concatenate([p.mu.values.reshape(n, 1), np.log(p.sigma.values).reshape(n, 1), np.log(p.nu.values).reshape(n, 1),
                           p.z.values.reshape(n, -1)], axis=1)
    want = c._expand_func(flat, **c._data)["volatility"]
    np.testing.assert_allclose(p.volatility.values.reshape(n, -1), np.asarray(want).reshape(n, -1), rtol=1e-12, atol=0)
