"""The Kalman smoother stage without a GPU (nutpie_amd/symbolic.py: kalman_smoothed_state; nutpie_amd/stage_families/kalman.py: the
``kalman_smooth`` op and its numpy evaluation; tests/fixtures/kalman_smoother_reference.c: the plain-C restatement of the device routine's
order contract) against the two mpmath forms of tests/kalman_smoother_reference.py.  DESIGN.md §11.9."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import kalman_models  # noqa: E402
import kalman_reference as K  # noqa: E402
import kalman_smoother_reference as KS  # noqa: E402

from nutpie_amd import density, stage_families as SF  # noqa: E402
from nutpie_amd import symbolic as S  # noqa: E402

ACCURACY_SHAPES = [(1, 3), (2, 20), (4, 65), (8, 200), (3, 500)]      # (m, T); three series, 15 % missing


def ir_smoother(R, T, m, values, masked, variance=False):
    """a Model whose operands are data, and kalman_smoothed_state of them -> (model, the value on product(steps, state))"""
    mod = S.Model()
    mod.dim("state", m)
    mod.dim("time", T)
    if R == 1:
        steps, along = "time", None
    else:
        mod.dim("series", R)
        steps, along = mod.product("series", "time").name, "time"
    zd, kk = mod.product(steps, "state"), mod.product("state", "state")
    dims = [steps, zd.name, steps, kk.name, kk.name, "state", kk.name]
    ops = [mod.data(n, np.reshape(values[k], -1), dim=d) for n, d, k in zip(["y", "Z", "h", "Tm", "Q", "a0", "P0"], dims, (0, 2, 3, 4, 5, 6, 7))]
    x = mod.param("unused")
    mod.add_logp(S.normal_lpdf(x, 0.0, 1.0))
    kw = dict(design=ops[1], obs_var=ops[2], transition=ops[3], state_cov=ops[4], init_mean=ops[5], init_cov=ops[6], along=along)
    if masked:
        kw["observed"] = mod.data("observed", np.reshape(values[1], -1), dim=steps)
    return mod, S.kalman_smoothed_state(ops[0], variance=variance, **kw), ops[0], kw


@pytest.fixture(scope="module")
def accuracy():
    """per shape: (inputs, the 50-digit reference, the same recursion at 53 bits, the C restatements' (F, S))"""
    R = 3
    out = {}
    for m, T in ACCURACY_SHAPES:
        values = K.inputs(R, T, m, seed=31 * m + T)      # (the inputs the filter's restatement is held to its bound on: test_kalman_cpu.py)
        out[m, T] = (values, KS.mp_sequential(*values, R, T, m), KS.mp_sequential(*values, R, T, m, prec=53), KS.filter_and_smooth(*values, R, T, m))
    return out


# --------------------------------------------------------------------------- 1. the reference: two independent forms
@pytest.mark.parametrize("m,T", [(1, 1), (1, 3), (2, 20), (4, 16), (8, 10)])
def test_the_sequential_and_the_dense_form_agree_to_1e40(m, T):
    """Series 0 misses its first step, series 1 its last, series 2 every step.  Q and P0 are made exactly symmetric: the recursion uses
    them as given, the dense form has no notion of an asymmetric covariance."""
    R = 3
    y, obs, Z, h, Tm, Q, a0, P0 = K.inputs(R, T, m, seed=10 * m + T)
    Q, P0 = (Q + Q.T) / 2.0, (P0 + P0.T) / 2.0
    obs[0, 0] = obs[1, -1] = 0.0
    obs[2, :] = 0.0
    assert (obs[0, 1:] == 1.0).any() or T == 1
    seq = KS.mp_sequential(y, obs, Z, h, Tm, Q, a0, P0, R, T, m)
    mean, var = KS.mp_dense(y, obs, Z, h, Tm, Q, a0, P0, R, T, m)
    e_mean, e_var = KS.rel_err(seq["asm"], mean), KS.rel_err(seq["vsm"], var)
    print(f"m = {m}, T = {T}: mean {e_mean:.3g}, variance {e_var:.3g}")
    assert e_mean <= 1e-40 and e_var <= 1e-40


# --------------------------------------------------------------------------- 2. accuracy of the C restatement
def test_c_restatement_is_as_accurate_as_the_recursion_in_double(accuracy):
    """The restatement (F from the filter's restatement) against the recursion at 50 digits, per array relative to the array's largest
    element; the bound is 4 x the error the same recursion makes when every operation is rounded to 53 bits, on the same inputs —
    the reference in double precision, not the code under test (the factor: §11.9's precedent).  Every shape and either array is held
    to its own bound; the inputs are those the filter's restatement is held to its bound on (seed 31 m + T).
    Measured, the worst shape of each: asm 3.49e-16 at (8, 200) (53 bits: 3.48e-16), vsm 4.88e-16 at (2, 20) (53 bits: 6.37e-16)."""
    for (m, T), (values, ref, dbl, (F, Sm)) in accuracy.items():
        n = 3 * T * m
        for name, got in (("asm", Sm[:n]), ("vsm", Sm[n:])):
            e_c, e_d = KS.rel_err(got, ref[name]), KS.rel_err(dbl[name], ref[name])
            print(f"m = {m}, T = {T}, {name}: C restatement {e_c:.3g}, recursion at 53 bits {e_d:.3g}, bound {4 * e_d:.3g}")
            assert e_d > 0.0
            assert e_c <= 4.0 * e_d, (m, T, name, e_c, e_d)


# --------------------------------------------------------------------------- 3. the numpy evaluation and the plumbing
@pytest.mark.parametrize("m,T", ACCURACY_SHAPES)
def test_numpy_evaluation_equals_the_restatement(m, T):
    """both packed arrays: 1e-13 of the array's largest element, without and with a mask (the filter's figure)"""
    R = 3
    values = K.inputs(R, T, m, seed=31 * m + T)
    y, obs, Z, h, Tm, Q, a0, P0 = values
    row = lambda v: np.reshape(np.asarray(v, dtype=np.float64), (1, -1))      # noqa: E731
    for masked in (False, True):
        F, want = KS.filter_and_smooth(y, obs if masked else None, Z, h, Tm, Q, a0, P0, R, T, m)
        got = S._np_kalman("kalman_smooth", [row(Z), row(Tm), row(F)] + ([row(obs)] if masked else []), R, T, m, masked, 1)[0]
        n = R * T * m
        for a, b in ((got[:n], want[:n]), (got[n:], want[n:])):
            assert np.abs(a - b).max() <= 1e-13 * np.abs(b).max()


@pytest.mark.parametrize("R,T,m,masked", [(1, 7, 2, True), (3, 5, 3, False), (2, 6, 1, True)])
def test_the_ir_value_is_the_restatement(R, T, m, masked):
    values = K.inputs(R, T, m, seed=R + 10 * T + 100 * m, missing=0.3)
    y, obs, Z, h, Tm, Q, a0, P0 = values
    _, want = KS.filter_and_smooth(y, obs if masked else None, Z, h, Tm, Q, a0, P0, R, T, m)
    n = R * T * m
    for variance, w in ((False, want[:n]), (True, want[n:])):
        mod, value, _, _ = ir_smoother(R, T, m, values, masked, variance)
        assert value.dim is mod.product(value.dim.factors[0].name, "state") and value.dim.size == n
        got = S.evaluate([value], np.zeros((2, 1)), mod._data)[0]
        assert got.shape == (2, n)
        assert np.abs(got - w).max() <= 1e-13 * np.abs(w).max()


def test_mean_and_variance_share_one_stage_on_the_density_s_filter():
    values = K.inputs(2, 6, 3, seed=1)
    mod, mean, y, kw = ir_smoother(2, 6, 3, values, True)
    var = S.kalman_smoothed_state(y, variance=True, **kw)
    lp = S.kalman_marginal_lpdf(y, **kw)
    nodes = S._topo([mean, var, lp])
    assert sum(n.op == "kalman_fwd" for n in nodes) == 1 and sum(n.op == "kalman_smooth" for n in nodes) == 1
    smooth = mean.args[0]
    assert smooth is var.args[0] and smooth.op == "kalman_smooth" and smooth.payload == (2, 6, 3, True)
    assert smooth.dim.name == "series_x_time__kf_s" and smooth.dim.size == 2 * 2 * 6 * 3 and len(smooth.args) == 4
    assert (mean.payload, var.payload) == (0, 2 * 6 * 3)
    assert SF.family_of("kalman_smooth") is SF.family_of("kalman_fwd") and S._KALOPS[-1] == "kalman_smooth"
    # a second smoother over the same steps with another state: dimensions named after the shape, as the filter's
    mod.dim("state2", 2)
    k2 = mod.product("state2", "state2")
    z2 = mod.data("Z2", np.ones(2), dim="state2")
    eye = mod.data("I2", np.eye(2).reshape(-1), dim=k2.name)
    other = S.kalman_smoothed_state(y, design=z2, obs_var=1.0, transition=eye, state_cov=eye, init_mean=0.0, init_cov=eye, along="time")
    assert other.args[0].dim.name == "series_x_time__kf_s_2x6x2" and other.args[0].args[2].dim.name == "series_x_time__kf_f_2x6x2"


def example_smoothed(x, mod, T, k=2):
    """the example's smoothed level and its standard deviation for the unconstrained positions ``x`` by the C restatements"""
    from nutpie_amd.timeseries import _trend_matrices

    Tm, z, p0 = _trend_matrices(None)
    level, sd, pred_var = [], [], []
    for row in np.atleast_2d(x):
        s = np.exp(row)
        F, Sm = KS.filter_and_smooth(mod._data["y"], mod._data["observed"], np.tile(z, T), np.full(T, s[0] * s[0]), Tm, np.diag([s[1] * s[1], s[2] * s[2]]),
                                     np.zeros(k), np.diag(p0), 1, T, k)
        level.append(Sm[:T * k].reshape(T, k)[:, 0])
        sd.append(np.sqrt(Sm[T * k:].reshape(T, k)[:, 0]))
        pred_var.append(F[T * k:T * k + T * k * k].reshape(T, k, k)[:, 0, 0])
    return np.array(level), np.array(sd), np.array(pred_var)


def test_the_example_s_deterministics_are_the_helper_on_the_same_arguments():
    T, ahead = 30, 4
    mod = kalman_models.example(T=T, smoothed=True, forecast=ahead)
    assert [n for n, _ in mod._det][-3:] == ["filtered_level", "smoothed_level", "smoothed_level_sd"]
    assert (mod._data["observed"][-ahead:] == 0.0).all() and mod._data["observed"].size == T + ahead
    x = kalman_models.points(mod, 5, seed=2)
    det = dict(mod._det)
    level, sd = S.evaluate([det["smoothed_level"], det["smoothed_level_sd"]], x, mod._data)
    want_level, want_sd, pred_var = example_smoothed(x, mod, T + ahead)
    assert level.shape == sd.shape == (5, T + ahead)
    assert np.abs(level - want_level).max() <= 1e-13 * np.abs(want_level).max()
    assert np.abs(sd - want_sd).max() <= 1e-13 * np.abs(want_sd).max()
    # the forecast: on the trailing missing steps the smoothed variance is the predicted one, and it grows with the horizon
    assert np.abs(sd[:, -ahead:] ** 2 - pred_var[:, -ahead:]).max() <= 1e-13 * pred_var.max()
    assert (np.diff(sd[:, -ahead:], axis=1) > 0.0).all()
    # the compiled model's host expand reports them
    out = mod.compile()._expand_func(x, **mod._data)
    assert np.array_equal(np.asarray(out["smoothed_level"]).reshape(5, -1), level)
    assert np.array_equal(np.asarray(out["smoothed_level_sd"]).reshape(5, -1), sd)


def test_a_result_too_long_for_the_expand_function_s_lds_is_expanded_on_the_host():
    """the rule of DESIGN.md §11.6 (``Family.long_results``): at T = 4000 the filter's and the smoother's packs pass the LDS of one
    workgroup, the model has no generated expand function, and the host reports the same values"""
    short, long_ = kalman_models.example(T=60, smoothed=True).compile(), kalman_models.example(T=4000, smoothed=True).compile()
    assert "nphip_expand" in short._source and "nphip_expand" not in long_._source and "nphip_kalman::forward<1, 4000, 2, true>(" in long_._source
    x = kalman_models.points(kalman_models.example(T=4000, smoothed=True), 1, seed=1)
    out = long_._expand_func(x, **long_._data)
    level, sd, _ = example_smoothed(x, kalman_models.example(T=4000, smoothed=True), 4000)
    assert np.abs(np.asarray(out["smoothed_level"]).reshape(1, -1) - level).max() <= 1e-13 * np.abs(level).max()
    assert np.abs(np.asarray(out["smoothed_level_sd"]).reshape(1, -1) - sd).max() <= 1e-13 * np.abs(sd).max()


# --------------------------------------------------------------------------- 4. identities
def test_missing_steps_report_the_prediction_exactly():
    """A series with every step missing, and the trailing missing steps of any series: asm == apred and vsm == diag(Ppred), in value,
    by the restatement and by the numpy evaluation."""
    R, T, m = 3, 12, 3
    y, obs, Z, h, Tm, Q, a0, P0 = K.inputs(R, T, m, seed=5)
    obs[0, :] = 0.0
    obs[1, -4:] = 0.0
    obs[1, -5] = 1.0
    obs[2, -1] = 1.0
    F, Sm = KS.filter_and_smooth(y, obs, Z, h, Tm, Q, a0, P0, R, T, m)
    row = lambda v: np.reshape(v, (1, -1))      # noqa: E731
    Fn = S._np_kalman("kalman_fwd", [row(v) for v in (y, Z, h, Tm, Q, a0, P0, obs)], R, T, m, True, 1)
    Sn = S._np_kalman("kalman_smooth", [row(Z), row(Tm), Fn, row(obs)], R, T, m, True, 1)
    n = R * T * m
    for F_, S_ in ((F, Sm), (Fn[0], Sn[0])):
        apred, Ppred = F_[:n].reshape(R, T, m), F_[n:n + n * m].reshape(R, T, m, m)
        mean, var = S_[:n].reshape(R, T, m), S_[n:].reshape(R, T, m)
        diag = np.einsum("rtii->rti", Ppred)
        assert np.array_equal(mean[0], apred[0]) and np.array_equal(var[0], diag[0])
        assert np.array_equal(mean[1, -4:], apred[1, -4:]) and np.array_equal(var[1, -4:], diag[1, -4:])
        assert not np.array_equal(mean[1, -5], apred[1, -5]) and (var[1, -5] < diag[1, -5]).all()


def test_last_step_is_the_filter_and_smoothing_never_adds_variance(accuracy):
    """With the last step observed the smoothed mean there is the filtered mean; a smoothed variance is at most the predicted one.  Both
    to the accuracy bound: 4 x the error of the recursion at 53 bits on the same inputs, relative to the array's largest element."""
    checked = 0
    for (m, T), (values, ref, dbl, (F, Sm)) in accuracy.items():
        R = 3
        n = R * T * m
        obs = values[1]
        afilt = F[n + n * m:2 * n + n * m].reshape(R, T, m)
        diag = np.einsum("rtii->rti", F[n:n + n * m].reshape(R, T, m, m))
        mean, var = Sm[:n].reshape(R, T, m), Sm[n:].reshape(R, T, m)
        b_mean = 4.0 * KS.rel_err(dbl["asm"], ref["asm"]) * np.abs(mean).max()
        b_var = 4.0 * KS.rel_err(dbl["vsm"], ref["vsm"]) * np.abs(var).max()
        for r in range(R):
            if obs[r, -1] != 0.0:
                assert np.abs(mean[r, -1] - afilt[r, -1]).max() <= b_mean, (m, T, r)
                checked += 1
        assert (var <= diag + b_var).all(), (m, T)
        assert (var > 0.0).all()
    assert checked >= 8


# --------------------------------------------------------------------------- 5. refusals
def test_a_gradient_through_the_result_is_refused():
    values = K.inputs(1, 5, 2, seed=3)
    mod, value, _, _ = ir_smoother(1, 5, 2, values, False)
    mod.add_logp(value.sum())
    with pytest.raises(NotImplementedError, match="kalman_smoothed_state carry no gradient"):
        S.gradient(mod.logp_expr(), mod._params)


def test_nine_states_are_refused_by_name_of_the_limit():
    values = K.inputs(1, 4, 9, seed=3)
    mod, value, _, _ = ir_smoother(1, 4, 9, values, False)
    mod.deterministic("path", value)
    with pytest.raises(ValueError, match="states of up to 8 dimensions"):
        mod.compile()


def test_malformed_shapes_raise():
    values = K.inputs(2, 5, 2, seed=3)
    mod, _, y, kw = ir_smoother(2, 5, 2, values, True)
    with pytest.raises(ValueError, match="kalman_smoothed_state: transition is an m x m value"):
        S.kalman_smoothed_state(y, **{**kw, "transition": kw["init_mean"]})
    with pytest.raises(ValueError, match="kalman_smoothed_state: along='week' names no axis"):
        S.kalman_smoothed_state(y, **{**kw, "along": "week"})
    with pytest.raises(ValueError, match="kalman_smoothed_state: 'series' is the outer axis"):
        S.kalman_smoothed_state(y, **{**kw, "along": "series"})
    with pytest.raises(ValueError, match="kalman_smoothed_state: observed is data"):
        S.kalman_smoothed_state(y, **{**kw, "observed": kw["obs_var"] * 2.0})
    with pytest.raises(ValueError, match="kalman_smoothed_state: y is a value or data on a fixed-size dimension"):
        S.kalman_smoothed_state(1.0, **kw)


# --------------------------------------------------------------------------- 6. models without the smoother are what they were
@pytest.mark.parametrize("which", ["trend", "ar"])
def test_a_model_without_a_smoothed_deterministic_does_not_know_the_header(which, monkeypatch):
    from nutpie_amd.timeseries import ar_p_model, local_linear_trend_model

    c = (local_linear_trend_model(50) if which == "trend" else ar_p_model(64, 3)).compile()
    assert "kalman_smoother.h" not in c._source and "kalman_smooth" not in c._source and "__kf_s" not in c._source
    assert SF.chain_headers(c._source) == ["chain_kalman.h", "chain_hmm.h"]
    key = density.library_key(c._source, density.data_layout(c._data), c._n_dim, waves=c._waves)[0]
    real_open = open

    def open_without_the_header(path, *a, **kw):
        return real_open(os.devnull if str(path).endswith("kalman_smoother.h") else path, *a, **kw)

    monkeypatch.setattr(density, "open", open_without_the_header, raising=False)
    assert density.library_key(c._source, density.data_layout(c._data), c._n_dim, waves=c._waves)[0] == key


def test_the_smoothed_example_includes_the_header_in_its_expand_function_only():
    from nutpie_amd.timeseries import local_linear_trend_model

    plain, smoothed = local_linear_trend_model(50).compile(), local_linear_trend_model(50, smoothed=True).compile()
    dens, expand = smoothed._source.split("nphip_expand")[0], smoothed._source.split("nphip_expand")[1]
    assert "nphip_kalman::smooth<1, 50, 2, true>(" in expand and "nphip_kalman::smooth" not in dens
    assert expand.count("nphip_kalman::forward<") == 1 and expand.count("nphip_kalman::smooth<") == 1
    assert SF.chain_headers(smoothed._source) == ["chain_kalman.h", "chain_hmm.h", "kalman_smoother.h"]
    # the density is the plain model's but for the length of the dimension the smoother adds (and the expand function's #include line, above its head)
    strip = lambda s: "\n".join(line for line in s.split("nphip_expand")[0].splitlines() if "__kf_s" not in line and "kalman_smoother.h" not in line)      # noqa: E731
    assert strip(smoothed._source) == strip(plain._source)
    key = lambda c: density.library_key(c._source, density.data_layout(c._data), c._n_dim, waves=c._waves)[0]      # noqa: E731
    assert key(smoothed) != key(plain)
