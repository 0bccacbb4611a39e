"""Matrix stages past 32 x 32 on the GPU (csrc/wide_chain_linalg.h, Model.compile(wide_matrices=True)): the five routines
against the CPU restatement of their order contract, tolerance zero, at 1, 2 and 4 waves per chain (tests/chain_stage_probes_wide.py: the
cases); a poisoned pivot stays in its chain; the generated models against the numpy evaluation, in the resident, batched and low-rank
forms; sharding; a deterministic on a wide factor; recovery of a GP length-scale on 100 points, as a model and as a traced torch density."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import chain_stage_probes as P  # noqa: E402
import chain_stage_probes_wide as PW  # noqa: E402
import matrix_models as mm  # noqa: E402

import nutpie_amd  # noqa: E402

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    """equal as bit patterns (so +0.0 is not -0.0), a NaN equal to any NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb])


def mismatches(probe, out, points, chains):
    bad = []
    for k, c in enumerate(probe.cases):
        for chain in chains:
            want, got = probe.expected(c, points[chain]), probe.got(out, c, chain)
            if not same_bits(got, want):
                diff = np.flatnonzero(~((got == want) & (np.signbit(got) == np.signbit(want)) | (np.isnan(got) & np.isnan(want))))
                bad.append(f"case {k} {c.name} [{c.mem}] chain {chain}: {diff.size} of {want.size} elements differ, first at {diff[0]}: {got[diff[0]]!r} != {want[diff[0]]!r}")
                break
    return bad


@pytest.mark.parametrize("W", [1, 2, 4])
def test_wide_routines_have_the_bits_of_the_restatement(hip, oracle, W):
    probe = PW.probe(W)
    points = P.clean_points()
    out = probe.run(points)
    assert np.isfinite(out).all()
    bad = mismatches(probe, out, points, range(P.N_CHAINS))
    assert not bad, f"{len(bad)} of {len(probe.cases)} cases:\n" + "\n".join(bad[:20])
    # the chains of one launch computed different numbers (the scale), so a chain that read its neighbour's scratch shows
    assert not np.array_equal(out[1], out[2])


@pytest.fixture(scope="module")
def contained_clean():
    return PW.containment_probe().run(P.clean_points())


@pytest.mark.parametrize("value", [-0.0, np.nan, np.inf, 5e-324])
def test_a_poisoned_pivot_stays_in_its_chain(hip, oracle, contained_clean, value):
    probe = PW.containment_probe()
    points = P.poisoned_points(value)
    out = probe.run(points)
    me = P.POISONED_CHAIN
    others = [c for c in range(P.N_CHAINS) if c != me]
    assert np.isfinite(contained_clean).all()
    assert same_bits(out[others], contained_clean[others])
    bad = mismatches(probe, out, points, [me])
    assert not bad, "\n".join(bad)
    for c in probe.cases:
        got = probe.got(out, c, me)
        K = c.p1.shape[0]
        if "diagonal" in c.name and value == 5e-324:      # a subnormal positive pivot factors
            assert np.isfinite(got).all() and got[c.poison[0]] == np.sqrt(5e-324) and np.count_nonzero(got) == K, c.name
        else:                                              # not a positive finite pivot (5e-324 less the earlier columns is negative)
            assert np.isnan(got).all(), c.name


def _points(c, n, seed):
    rng = np.random.default_rng(seed)
    K = c.n_dim - 3
    return np.concatenate([rng.normal([-0.2, -0.4, -1.5], 0.2, size=(n, 3)), 0.3 * rng.normal(size=(n, K))], axis=1)


@pytest.mark.parametrize("K,N,W", [(33, 1, None), (33, 85, None), (64, 1, None), (64, 85, None), (128, 1, None), (128, 85, None), (128, 1, 4)])
def test_generated_wide_stages_equal_the_numpy_evaluation(hip, K, N, W):
    c = mm.gp_rows(K, N).compile(wide_matrices=True, waves_per_chain=W)
    assert "nphip_lw::cholesky" in c._source and (W is None or c._waves == W)
    x = _points(c, 64, K * 1000 + N)
    lp, g = c.logp_and_grad(x)
    lp_ref, g_ref = c.logp_and_grad_numpy(x)
    print(f"K={K} N={N} W={c._waves}: logp {np.max(np.abs(lp - lp_ref) / np.abs(lp_ref)):.2e} rel, grad {np.max(np.abs(g - g_ref)):.2e} abs of {np.abs(g_ref).max():.2e}")
    np.testing.assert_allclose(lp, lp_ref, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(g, g_ref, rtol=1e-8, atol=1e-8 * np.abs(lp_ref).max())


@pytest.mark.parametrize("adaptation", ["diag", "low_rank"])
def test_resident_and_batched_forms_draw_the_same(hip, adaptation):
    m = mm.gp_rows(64, 1)
    kw = dict(chains=32, tune=100, draws=40, seed=5, progress_bar=False, adaptation=adaptation)
    a = nutpie_amd.sample(m.compile(wide_matrices=True), **kw)
    b = nutpie_amd.sample(m.compile(wide_matrices=True, resident=False), **kw)
    assert np.array_equal(a.posterior.mu.values, b.posterior.mu.values)
    assert np.array_equal(a.sample_stats.n_steps.values, b.sample_stats.n_steps.values)
    assert np.all(np.isfinite(a.posterior.log_ls.values))


def test_chain_sharding_invariance(hip):
    c = mm.gp_rows(64, 1).compile(wide_matrices=True)
    kw = dict(tune=100, draws=40, seed=17, progress_bar=False)
    big = nutpie_amd.sample(c, chains=64, **kw)
    small = nutpie_amd.sample(c, chains=8, **kw)
    assert np.array_equal(big.posterior.mu.values[:8], small.posterior.mu.values)
    assert np.array_equal(big.posterior.log_amp.values[:8], small.posterior.log_amp.values)


def test_a_deterministic_on_a_wide_factor(hip):
    c = mm.gp_rows(40, 2, factor_deterministic=True).compile(wide_matrices=True)
    tr = nutpie_amd.sample(c, chains=16, tune=100, draws=30, seed=3, progress_bar=False)
    p = tr.posterior
    n = p.log_amp.values.size
    flat = np.concatenate([p.log_amp.values.reshape(n, 1), p.log_ls.values.reshape(n, 1), p.log_noise.values.reshape(n, 1), p.mu.values.reshape(n, -1)], axis=1)
    want = c._expand_func(flat, **c._data)["cov_chol"]       # the numpy evaluation of the same draws
    np.testing.assert_allclose(p.cov_chol.values.reshape(n, -1), np.asarray(want).reshape(n, -1), rtol=1e-12, atol=1e-14)


GP = dict(n=100, length_scale=0.8, amplitude=1.0, noise=0.2)


def _covers_its_length_scale(tr, log_ls):
    assert tr.sample_stats.diverging.values.sum() == 0
    lo, hi = np.quantile(np.exp(log_ls).reshape(-1), [0.005, 0.995])
    print(f"length-scale interval [{lo:.3f}, {hi:.3f}]")
    assert lo < GP["length_scale"] < hi


def test_gp_example_recovers_its_length_scale(hip):
    from nutpie_amd import gp

    c = gp.compile_gp_regression(*gp.synthetic_gp(**GP))
    assert "nphip_lw::cholesky<100>(" in c._source
    tr = nutpie_amd.sample(c, chains=64, tune=300, draws=150, seed=4, progress_bar=False)
    _covers_its_length_scale(tr, tr.posterior.log_ls.values)


def test_traced_gp_example_recovers_its_length_scale(hip):
    from nutpie_amd import gp

    D, logp = gp.gp_regression_torch_density(*gp.synthetic_gp(**GP))
    model = nutpie_amd.from_torch_density(D, logp, compile=True, wide_matrices=True)
    assert "nphip_lw::cholesky<100>(" in model._source
    tr = nutpie_amd.sample(model, chains=64, tune=300, draws=150, seed=4, progress_bar=False)
    _covers_its_length_scale(tr, tr.posterior.x.values[..., 1])
