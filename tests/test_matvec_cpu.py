"""Products with a wide design matrix in the symbolic IR (the matvec / matvec_t stages of symbolic.Matrix): the numpy evaluation against
a Python double loop, the symbolic gradient against central differences and torch.autograd, both lowerings of one model against each
other, the torch front end, the generated source, with_data, and cross-compilation of the device routine (csrc/chain_matvec.h) at
one, two and four waves per chain."""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import regression_models as rm  # noqa: E402

from nutpie_amd import symbolic as S  # noqa: E402


def test_sources_of_narrow_design_matrices_are_unchanged():
    # (the hashes of the sources these models generated before the stage existed)
    import symbolic_models
    import torch_models

    from nutpie_amd.torch_trace import trace

    def h(c):
        assert "chain_matvec" not in c._source and "nphip_mv::" not in c._source
        return hashlib.sha256(c._source.encode()).hexdigest()

    assert h(symbolic_models.regression().compile()) == "abd4cef4a24a67d3c5370a11934d90c7ea58fbc0a1fa8302fdfb8c263d38c15e"
    assert h(symbolic_models.plain_regression().compile()) == "48905b7fc5973223d16c7340cb8cd57f984ebd0482caa28843f107af4ae9ad8e"
    assert h(symbolic_models.collinear_regression().compile()) == "e4c04a883a5fca8b89614c3f4bd97d6bc5fcef3753b52413609c4cc73b525caa"
    for name, want in (("logistic_regression", "6ffd605f03f357eeb31c686584c0b5685883f5ca25e43be2811c25f4439e8bcc"),
                       ("linear_regression_unbatched", "f14359931b262386387fbfe79d9b93c8262163906f28dc25833175a33db41fba"),
                       ("negbin_and_pairwise", "7d10ae563eafedc05c12df3a2042207a663dfe443e94e97b1966ec01178d5c85")):
        D, fn, batched, shared = getattr(torch_models, name)()
        assert h(trace(fn, D, batched=batched, shared_data=shared).compile()) == want, name


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2000])
@pytest.mark.parametrize("k", [33, 64, 200])
def test_numpy_evaluation_equals_a_double_loop(n, k):
    rng = np.random.default_rng(n + k)
    Xv = rng.normal(size=(n, k))
    m = S.Model()
    b = m.param("b", dim="coef", size=k)
    X = m.matrix("X", Xv, dim="obs", cols="coef", stage=True)       # (k = 33 is below the automatic threshold)
    g = m.data("g", rng.normal(size=n), dim="obs")
    e, c = X @ b, X.T @ (g * g)
    assert (e.op, e.dim.name, c.op, c.dim.name) == ("matvec", "obs", "matvec_t", "coef")
    x = rng.normal(size=(2, k))
    ev, cv = S.evaluate([e, c], x, m._data)
    gg = m._data["g"] ** 2
    # rtol 1e-13, plus 1e-13 of the LARGEST element as an absolute term: an element of X b is a sum of k terms of either sign, and one
    # that cancels to a small value carries the rounding of terms far larger than itself (without the term: up to 3.9e-13 relative on
    # such elements at k = 200, 1.1e-14 absolute, between einsum's and the loop's orders of summation)
    for p in range(2):
        want_e = [sum(Xv[i, j] * x[p, j] for j in range(k)) for i in range(n)]
        np.testing.assert_allclose(ev[p], want_e, rtol=1e-13, atol=1e-13 * np.abs(want_e).max())
    want_c = [sum(Xv[i, j] * gg[i] for i in range(n)) for j in range(k)]
    np.testing.assert_allclose(cv[0], want_c, rtol=1e-13, atol=1e-13 * np.abs(want_c).max())


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2000])
@pytest.mark.parametrize("k", [33, 64, 200])
def test_numpy_evaluation_with_three_right_hand_sides_equals_a_double_loop(n, k):
    R = 3
    rng = np.random.default_rng(n + k)
    Xv = rng.normal(size=(n, k))
    m = S.Model()
    m.dim("coef", k)
    m.dim("rhs", R)
    B = m.param("B", dims=("coef", "rhs"))
    X = m.matrix("X", Xv, dim="obs", cols="coef")
    E = X @ B
    assert (E.op, E.dim.name, E.payload) == ("matvec", "obs_x_rhs", ("X", k, R)) and E.dim.len_py(m._data) == n * R
    G = m.data("G", rng.normal(size=n * R), dim=E.dim.name)
    C = X.T @ (G * G)
    assert (C.op, C.dim.name) == ("matvec_t", "coef_x_rhs")
    x = rng.normal(size=(1, k * R))
    ev, cv, col = S.evaluate([E, C, S.column(E, 2)], x, m._data)
    Bv, GG = x[0].reshape(k, R), (m._data["G"] ** 2).reshape(n, R)
    want_e = np.array([[sum(Xv[i, j] * Bv[j, r] for j in range(k)) for r in range(R)] for i in range(n)])
    want_c = np.array([[sum(Xv[i, j] * GG[i, r] for i in range(n)) for r in range(R)] for j in range(k)])
    # (the absolute term: as in the test above — elements that cancel)
    np.testing.assert_allclose(ev[0], want_e.reshape(-1), rtol=1e-13, atol=1e-13 * np.abs(want_e).max())
    np.testing.assert_allclose(cv[0], want_c.reshape(-1), rtol=1e-13, atol=1e-13 * np.abs(want_c).max())
    np.testing.assert_array_equal(col[0], ev[0].reshape(n, R)[:, 2])


def _central(c, x, h=1e-6):
    g = np.zeros_like(x)
    for k in range(x.shape[1]):
        e = np.zeros(x.shape[1])
        e[k] = h
        g[:, k] = (c.logp_and_grad_numpy(x + e)[0] - c.logp_and_grad_numpy(x - e)[0]) / (2 * h)
    return g


def _examples(name, n=120, k=64):
    from nutpie_amd import regression as R

    if name == "logistic":
        X, y = rm.logistic_data(n, k)
        return R.logistic_regression_model(X, y), R.logistic_regression_torch_density(X, y)
    if name == "softmax":
        X, y = rm.softmax_data(n, k, 4)
        return R.softmax_regression_model(X, y, 4), R.softmax_regression_torch_density(X, y, 4)
    X, y = rm.gaussian_data(n, k)
    return R.horseshoe_regression_model(X, y), R.horseshoe_regression_torch_density(X, y)


@pytest.mark.parametrize("example", ["logistic", "horseshoe", "softmax"])
def test_gradient_of_the_examples_matches_central_differences_and_autograd(example):
    import torch

    model, (D, logp) = _examples(example)
    c = model.compile()
    assert '#include "chain_matvec.h"' in c._source and c.n_dim == D
    x = rm.points(D, 3, seed=5)
    lp, g = c.logp_and_grad_numpy(x)
    np.testing.assert_allclose(g, _central(c, x), rtol=1e-6, atol=1e-6 * np.abs(g).max())
    xt = torch.tensor(x, requires_grad=True)
    lt = logp(xt)
    lt.sum().backward()
    np.testing.assert_allclose(lp, lt.detach().numpy(), rtol=1e-12)
    np.testing.assert_allclose(g, xt.grad.numpy(), rtol=1e-12, atol=1e-13)


def test_gradient_of_a_direct_transposed_product_matches_central_differences():
    c = rm.probe_model(70, 33, seed=2).compile()
    assert c._source.count("nphip_mv::times<33, 1>") == 2 and c._source.count("nphip_mv::times_t<33, 1>") == 2
    x = rm.points(c.n_dim, 2, seed=3)
    _, g = c.logp_and_grad_numpy(x)
    np.testing.assert_allclose(g, _central(c, x), rtol=1e-6, atol=1e-6 * np.abs(g).max())


def test_gradient_through_both_products_with_several_right_hand_sides_matches_central_differences():
    c = rm.probe_model_rhs(70, 33, 3, seed=2).compile()
    assert c._source.count("nphip_mv::times<33, 3>") == 2 and c._source.count("nphip_mv::times_t<33, 3>") == 2
    x = rm.points(c.n_dim, 2, seed=3)
    _, g = c.logp_and_grad_numpy(x)
    np.testing.assert_allclose(g, _central(c, x), rtol=1e-6, atol=1e-6 * np.abs(g).max())


def test_both_lowerings_of_one_model_agree():
    a, b = rm.gaussian_model(300, 40, stage=True).compile(), rm.gaussian_model(300, 40, stage=False).compile()
    assert "nphip_mv::" in a._source and "nphip_mv::" not in b._source
    assert "nphip_mv::" in rm.gaussian_model(300, 64).compile()._source          # (automatic: from 64 columns on)
    assert "nphip_mv::" not in rm.gaussian_model(300, 63).compile()._source
    x = rm.points(a.n_dim, 4, seed=1)
    (la, ga), (lb, gb) = a.logp_and_grad_numpy(x), b.logp_and_grad_numpy(x)
    np.testing.assert_allclose(la, lb, rtol=1e-12)
    np.testing.assert_allclose(ga, gb, rtol=1e-12, atol=1e-12 * np.abs(gb).max())


def test_the_source_calls_each_routine_once_and_does_not_grow_with_the_columns():
    # four waves per chain: the element-wise loops over the 64 resp. 200 coefficients then take one trip of 256 lanes in both models
    # (the generator unrolls a loop over a fixed-size dimension by its trips, up to four: with fewer waves the k = 200 source has the
    # bodies of those loops two resp. four times — that, not the product, is all that differs, and it is bounded below as well)
    src = {k: rm.logistic(2000, k).compile(waves_per_chain=4)._source for k in (64, 200)}
    assert '#include "chain_matvec.h"' in src[200]
    assert src[200].count("nphip_mv::times<200, 1>") == 1 and src[200].count("nphip_mv::times_t<200, 1>") == 1
    assert abs(len(src[200]) - len(src[64])) < 0.01 * len(src[64])
    # (one wave per chain: 200 and 256 coefficients both take four trips of 64 lanes)
    one = {k: rm.logistic(2000, k).compile(waves_per_chain=1)._source for k in (200, 256)}
    assert one[200].count("nphip_mv::times<200, 1>") == 1 and one[200].count("nphip_mv::times_t<200, 1>") == 1
    assert abs(len(one[256]) - len(one[200])) < 0.01 * len(one[200])
    src = one
    # the matrix and its transposed copy are read from device memory, the rest of the data from LDS
    assert "(data.X__t, " in src[200] and "(data.X, " in src[200] and "D_X" not in src[200]
    assert "const auto D_y = NPHIP_LDS_CPTR(double" in src[200]


def test_a_traced_wide_logistic_regression_keeps_the_matrix_as_data():
    import torch

    from nutpie_amd.regression import logistic_regression_torch_density
    from nutpie_amd.torch_trace import trace

    n, k = 2000, 200
    X, y = rm.logistic_data(n, k)
    D, logp = logistic_regression_torch_density(X, y)
    t = trace(logp, D)
    assert max(d.len_py(t.model._data) for d in t.model._dims.values()) <= max(n, k)
    assert sum(np.size(v) for v in t.model._data.values()) < 2 * n * k + 10 * (n + k)
    c = t.compile()
    assert "nphip_mv::times<200, 1>" in c._source and "nphip_mv::times_t<200, 1>" in c._source
    x = rm.points(D, 3, seed=8)
    lp, g = c.logp_and_grad_numpy(x)
    xt = torch.tensor(x, requires_grad=True)
    lt = logp(xt)
    lt.sum().backward()
    np.testing.assert_allclose(lp, lt.detach().numpy(), rtol=1e-12)
    np.testing.assert_allclose(g, xt.grad.numpy(), rtol=1e-12, atol=1e-13)


def test_a_traced_softmax_regression_is_one_product_with_four_right_hand_sides():
    import torch

    from nutpie_amd.regression import softmax_regression_torch_density
    from nutpie_amd.torch_trace import trace

    n, k, R = 2000, 200, 4
    X, y = rm.softmax_data(n, k, R)
    D, logp = softmax_regression_torch_density(X, y, R)
    t = trace(logp, D)
    assert max(d.len_py(t.model._data) for d in t.model._dims.values()) <= max(n, k) * R
    c = t.compile()
    assert "nphip_mv::times<200, 4>" in c._source and "nphip_mv::times_t<200, 4>" in c._source
    x = rm.points(D, 2, seed=8)
    lp, g = c.logp_and_grad_numpy(x)
    xt = torch.tensor(x, requires_grad=True)
    lt = logp(xt)
    lt.sum().backward()
    np.testing.assert_allclose(lp, lt.detach().numpy(), rtol=1e-12)
    np.testing.assert_allclose(g, xt.grad.numpy(), rtol=1e-12, atol=1e-13)


def test_with_data_rederives_the_transposed_copy():
    c = rm.logistic(150, 40, stage=True).compile()
    X2, y2 = rm.logistic_data(90, 40, seed=4)
    c2 = c.with_data(X=X2, y=y2)
    np.testing.assert_array_equal(c2._data["X__t"].reshape(40, 90), X2.T)
    fresh = rm.logistic(90, 40, seed=4, stage=True).compile()
    x = rm.points(c.n_dim, 3, seed=2)
    np.testing.assert_allclose(c2.logp_and_grad_numpy(x)[0], fresh.logp_and_grad_numpy(x)[0], rtol=1e-14)
    np.testing.assert_allclose(c2.logp_and_grad_numpy(x)[1], fresh.logp_and_grad_numpy(x)[1], rtol=1e-14)
    # the same number of rows: no new source, the copy follows all the same
    X3, _ = rm.logistic_data(150, 40, seed=9)
    np.testing.assert_array_equal(c.with_data(X=X3)._data["X__t"].reshape(40, 150), X3.T)
    with pytest.raises(ValueError, match="40 columns"):
        c.with_data(X=np.zeros((150, 41)))
    with pytest.raises(ValueError, match="Unknown data"):
        c.with_data(X__t=np.zeros(150 * 40))


@pytest.mark.parametrize("W", [1, 2, 4])
def test_wide_logistic_density_compiles_for_gfx950(W):
    from nutpie_amd.density import compile_density, data_layout

    c = rm.logistic(2000, 200).compile(waves_per_chain=W)
    assert os.path.exists(compile_density(c._source, data_layout(c._data), c.n_dim, waves=W))


@pytest.mark.parametrize("W", [1, 2, 4])
def test_softmax_density_compiles_for_gfx950(W):
    from nutpie_amd.density import compile_density, data_layout
    from nutpie_amd.regression import softmax_regression_model

    X, y = rm.softmax_data(2000, 50, 4)
    c = softmax_regression_model(X, y, 4).compile(waves_per_chain=W)
    assert "nphip_mv::times<50, 4>" in c._source and "nphip_mv::times_t<50, 4>" in c._source
    assert os.path.exists(compile_density(c._source, data_layout(c._data), c.n_dim, waves=W))


def test_with_data_of_another_length_follows_through_a_product_with_data_rows():
    from nutpie_amd.regression import softmax_regression_model

    X, y = rm.softmax_data(120, 40, 3)
    X2, y2 = rm.softmax_data(75, 40, 3, seed=5)
    c = softmax_regression_model(X, y, 3).compile()
    c2 = c.with_data(X=X2, y_onehot=np.eye(3)[y2].reshape(-1))
    fresh = softmax_regression_model(X2, y2, 3).compile()
    x = rm.points(c.n_dim, 3, seed=2)
    np.testing.assert_allclose(c2.logp_and_grad_numpy(x)[0], fresh.logp_and_grad_numpy(x)[0], rtol=1e-14)
    with pytest.raises(ValueError, match="share one length"):
        c.with_data(X=X2)


def test_forced_stage_and_malformed_products():
    c = rm.gaussian_model(50, 8, stage=True).compile()
    assert "nphip_mv::times<8, 1>" in c._source
    x = rm.points(c.n_dim, 2, seed=1)
    ref = rm.gaussian_model(50, 8).compile()
    assert "nphip_mv::" not in ref._source
    np.testing.assert_allclose(c.logp_and_grad_numpy(x)[1], ref.logp_and_grad_numpy(x)[1], rtol=1e-12, atol=1e-13)
    m = S.Model()
    X = m.matrix("X", np.ones((20, 40)), dim="obs", cols="coef")
    other = m.param("v", dim="other", size=40)
    on_rows = m.data("g", np.ones(20), dim="obs")
    with pytest.raises(ValueError, match="'X'"):
        X @ other
    with pytest.raises(ValueError, match="'X'"):
        X @ on_rows
    with pytest.raises(ValueError, match="'X'"):
        X.T @ other
    with pytest.raises(ValueError, match="'X'"):
        X @ 2.0
    m.dim("many", 17)
    m.dim("few", 3)
    with pytest.raises(ValueError, match="'X'.*16 right-hand sides"):
        X @ m.param("B17", dims=("coef", "many"))
    with pytest.raises(ValueError, match="'X'"):
        X @ m.param("Bt", dims=("few", "coef"))          # (the first factor is not the matrix's columns)
    E = X @ m.param("B3", dims=("coef", "few"))
    assert E.payload == ("X", 40, 3) and E.dim.factors[0].name == "obs"
    with pytest.raises(ValueError, match="data rows"):
        m.reduce(E, over="few")


def test_staging_does_not_count_the_matrices_that_only_stages_read():
    m = rm.logistic(2000, 200)
    c = m.compile(waves_per_chain=2)
    f = c._front
    assert f._unstaged == {"X", "X__t"} and f._staged          # (3.2 MB of matrix; y alone is staged)
    assert f._shared_doubles(f._data) == 2000
    # the same matrix through the sum over its columns is staged data, and too large for it
    assert not rm.logistic(2000, 200, stage=False).compile(waves_per_chain=2)._front._staged


def test_deterministics_on_both_sides_of_the_stages():
    c = rm.reporting_model(90, 40).compile()
    x = rm.points(c.n_dim, 3, seed=1)
    out = c._expand_func(x, **c._data)
    X, y = c._data["X"].reshape(90, 40), c._data["y"]
    mu = x[:, :1] + x[:, 2:] @ X.T
    np.testing.assert_allclose(out["mu"], mu, rtol=1e-13, atol=1e-14)
    np.testing.assert_allclose(out["score"], (y - mu) @ X, rtol=1e-12, atol=1e-13)
    # (mu lives on a data dimension: the model expands on the host; without it the values on fixed-size dimensions are generated code)
    assert "nphip_expand" not in c._source
    assert "nphip_mv::times_t<40, 1>" in rm.reporting_model(90, 40, report_mu=False).compile()._source.split("nphip_expand")[1]


@pytest.mark.parametrize("W", [1, 4])
def test_a_narrow_matrix_read_by_the_loops_and_by_a_stage_compiles_for_gfx950(W):
    # 8 columns: `X @ beta` is the sum over the columns, whose loops read the matrix from the staged copy in LDS, `X.T @ g` the stage,
    # which reads it from device memory
    from nutpie_amd.density import compile_density, data_layout

    c = rm.probe_model(50, 8, stage=None).compile(waves_per_chain=W)
    assert c._front._staged and "X" not in c._front._unstaged
    assert "const auto D_X = NPHIP_LDS_CPTR(double" in c._source and "nphip_mv::times_t<8, 1>(data.X, " in c._source
    assert "nphip_mv::times<8, 1>(data.X__t, " in c._source          # (the adjoint of the transposed product)
    x = rm.points(c.n_dim, 2, seed=3)
    _, g = c.logp_and_grad_numpy(x)
    np.testing.assert_allclose(g, _central(c, x), rtol=1e-6, atol=1e-6 * np.abs(g).max())
    assert os.path.exists(compile_density(c._source, data_layout(c._data), c.n_dim, waves=W))


def test_columns_of_a_product_with_data_rows_and_their_errors():
    m = S.Model()
    m.dim("coef", 40)
    m.dim("few", 3)
    X = m.matrix("X", np.arange(80.0).reshape(2, 40), dim="obs", cols="coef")
    E = X @ m.param("B", dims=("coef", "few"))
    v = m.data("v", np.array([1.0, 2.0]), dim="obs")
    P = S.pack_columns([v, 2.0 * v, 0.5], E.dim)
    assert S.column(P, 1) is 2.0 * v and S.column(E, 2).dim.name == "obs"
    assert S.pack_columns([0.0, 0.0, 0.0], E.dim).is_const(0.0)
    np.testing.assert_array_equal(S.evaluate([P], np.zeros((1, 120)), m._data)[0][0], [1.0, 2.0, 0.5, 2.0, 4.0, 0.5])
    with pytest.raises(ValueError, match="column"):
        S.column(E, 3)
    with pytest.raises(ValueError, match="column"):
        S.column(v, 0)
    with pytest.raises(ValueError, match="pack_columns"):
        S.pack_columns([v, v], E.dim)
    with pytest.raises(ValueError, match="pack_columns"):
        S.pack_columns([v, v, m.param("w", dim="few")], E.dim)
    with pytest.raises(ValueError, match="pack_columns"):
        S.pack_columns([v, v, v], X.dim)
    with pytest.raises(ValueError, match="data rows"):
        m.broadcast(v, "obs", "few")
    with pytest.raises(ValueError, match="a product needs"):
        m.product("few", "obs")
    # a reported value on the product: the host expand gives it its (rows, right-hand sides) shape, also after with_data
    m.add_logp(S.normal_lpdf(E, 0.0, 1.0).sum())
    m.deterministic("E", E)
    c = m.compile()
    x = rm.points(c.n_dim, 2, seed=1)
    out = c._expand_func(x, **c._data)["E"]
    want = np.einsum("ik,nkr->nir", np.arange(80.0).reshape(2, 40), x[:, :120].reshape(2, 40, 3))       # (x also holds the 3 of `w`)
    np.testing.assert_allclose(out, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
    c3 = c.with_data(X=np.ones((5, 40)), v=np.ones(5))
    assert c3._expand_func(x, **c3._data)["E"].shape == (2, 5, 3)
