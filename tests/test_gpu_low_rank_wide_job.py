"""adaptation="low_rank" end to end at 300 dimensions: 64 basis draws, so the windows go to nphip_low_rank_estimate_wide and the job takes
the fast driver — the torch estimator is never called, the job is reproducible from its seed bit for bit, and the metric does its work."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D = 300


@pytest.fixture(scope="module")
def jobs(hip):
    import nutpie_amd
    from nutpie_amd import low_rank as lr

    native, calls = [], []
    real_native, real_estimate = lr.LowRankSampler._native_estimator, lr.estimate

    def native_spy(self):
        native.append(real_native(self))
        return native[-1]

    def estimate_spy(*a, **k):
        calls.append(1)
        raise AssertionError("low_rank.estimate was called: the windows did not go to the estimator kernel")

    mp = pytest.MonkeyPatch()
    mp.setattr(lr.LowRankSampler, "_native_estimator", native_spy)
    mp.setattr(lr, "estimate", estimate_spy)
    try:
        m = nutpie_amd.ar1_gaussian(D, rho=0.995, scales=np.ones(D))
        kw = dict(chains=32, tune=400, draws=200, seed=5, progress_bar=False)
        runs = [nutpie_amd.sample(m, adaptation="low_rank", mass_matrix_eigval_cutoff=1.5, **kw) for _ in range(2)]
        dg = nutpie_amd.sample(m, adaptation="diag", **kw)
    finally:
        mp.undo()
    assert real_estimate is lr.estimate
    return dict(runs=runs, diag=dg, native=native, calls=calls)


def test_the_job_takes_the_estimator_kernel_and_never_the_torch_formulation(hip, jobs):
    from nutpie_amd import low_rank as lr

    assert lr.basis_draws_for(D) == 64 and not hip.low_rank_estimate_supported(D, lr.WINDOW_MAX, 64, lr.K_MAX)
    assert hip.low_rank_estimate_wide_supported(D, lr.WINDOW_MAX, 64, lr.K_MAX)
    assert jobs["native"] and all(jobs["native"])
    assert jobs["calls"] == []


def test_two_runs_from_one_seed_are_equal_bit_for_bit(jobs):
    a, b = jobs["runs"]
    assert np.array_equal(a.posterior.x.values, b.posterior.x.values)
    assert np.array_equal(a.warmup_posterior.x.values, b.warmup_posterior.x.values)
    for key in ("n_steps", "diverging", "energy", "step_size", "logp"):
        if key in a.sample_stats:
            assert np.array_equal(a.sample_stats[key].values, b.sample_stats[key].values), key
    assert "n_steps" in a.sample_stats and "diverging" in a.sample_stats


def test_the_metric_shortens_the_trees_and_the_posterior_is_right(jobs):
    """The marginal sds are within 0.2 of 1: the tolerance of the D = 48 job of tests/test_gpu_low_rank.py (6400 draws of a chain
    with correlation 0.995 between neighbours)."""
    lr_, dg = jobs["runs"][0], jobs["diag"]
    steps_lr, steps_dg = float(lr_.sample_stats.n_steps.values.mean()), float(dg.sample_stats.n_steps.values.mean())
    x = lr_.posterior.x.values.reshape(-1, D)
    dev_lr = float(np.abs(x.std(0) - 1).max())
    dev_dg = float(np.abs(dg.posterior.x.values.reshape(-1, D).std(0) - 1).max())
    div = float(lr_.sample_stats.diverging.values.mean())
    print("low_rank_wide_job D %d leapfrogs per draw low_rank %.1f diag %.1f  max |sd - 1| low_rank %.3f diag %.3f  divergences %.4f"
          % (D, steps_lr, steps_dg, dev_lr, dev_dg, div))
    assert div < 0.01
    assert steps_lr < steps_dg, (steps_lr, steps_dg)
    assert dev_lr < 0.2, (dev_lr, dev_dg)
