"""The Kalman smoother in compiled models on the GPU (nutpie_amd/symbolic.py: kalman_smoothed_state; csrc/kalman_smoother.h inside the
generated expand function): the example's smoothed level and its standard deviation from the device expand against the host, forecasts
included, and the law of the smoothed state against the same model with its latent path as parameters.  DESIGN.md §11.9."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import kalman_models  # noqa: E402
import kalman_smoother_reference as KS  # noqa: E402

import nutpie_amd  # noqa: E402

pytestmark = pytest.mark.gpu

SMOOTHED_EXAMPLE, LAW, local_level_smoothed = KS.SMOOTHED_EXAMPLE, KS.LAW, KS.local_level_smoothed
SCALES = ("sigma_obs_log__", "sigma_level_log__", "sigma_slope_log__")


def reported_references(mod, u):
    """for the unconstrained draws ``u`` of the example: the 50-digit level, its sd and the sd of the predicted level [draw, T] as floats,
    and the errors of the same recursion at 53 bits (the level relative to the largest level, either sd to the largest smoothed sd)"""
    import mpmath

    from nutpie_amd.timeseries import _trend_matrices

    Tm, z, p0 = _trend_matrices(None)
    T = mod._data["y"].size
    level, sd, pred_sd, e_level, e_sd = [], [], [], 0.0, 0.0
    for row in u:
        s = np.exp(row)
        args = (mod._data["y"], mod._data["observed"], np.tile(z, T), np.full(T, s[0] * s[0]), Tm, np.diag([s[1] * s[1], s[2] * s[2]]), np.zeros(2), np.diag(p0), 1, T, 2)
        ref, dbl = KS.mp_sequential(*args), KS.mp_sequential(*args, prec=53)
        with mpmath.workdps(KS.DIGITS):
            ref_sd = [mpmath.sqrt(v) for v in ref["vsm"][0, :, 0]]
            ref_pred = [mpmath.sqrt(v) for v in ref["Ppred"][0, :, 0, 0]]
        with mpmath.workprec(53):
            dbl_sd = [mpmath.sqrt(v) for v in dbl["vsm"][0, :, 0]]
        e_level, e_sd = max(e_level, KS.rel_err(dbl["asm"][0, :, 0], ref["asm"][0, :, 0])), max(e_sd, KS.rel_err(dbl_sd, ref_sd))
        level.append([float(v) for v in ref["asm"][0, :, 0]])
        sd.append([float(v) for v in ref_sd])
        pred_sd.append([float(v) for v in ref_pred])
    return np.array(level), np.array(sd), np.array(pred_sd), e_level, e_sd


@pytest.fixture(scope="module")
def references():
    return {}


@pytest.mark.parametrize("W", [1, 2])
def test_smoothed_level_from_the_device_expand_equals_the_host(hip, W, references):
    """The compiled example with ``smoothed=True`` (T = 50, 10 % missing, 5 trailing missing steps): ``smoothed_level`` and
    ``smoothed_level_sd`` of the device expand against the host evaluation of the same draws, and on the trailing steps the sd
    against the predicted one.  The bound, for each reported array: 4 x the error of the 53-bit recursion (mpmath, against the same
    recursion at 50 digits; for an sd followed by a 53-bit square root) relative to the array's largest element, the worst of the
    draws — the reference in double precision, as for the C restatement (tests/test_kalman_smoother_cpu.py).  The sd squared is
    the predicted variance: stated for the reported quantity, the sd against the root of the predicted variance.
    Measured (W = 1 and 2 alike): level, device - host 4.4e-14 for a bound of 1.5e-13 (the 53-bit recursion loses 2.2e-15 of 17.1: P0 =
    100); sd 3.9e-12 for 1.1e-10 (vsm = P - (P N) P cancels against P0 at the first steps); forecast sd 6.7e-16."""
    mod = kalman_models.example(**SMOOTHED_EXAMPLE)
    c = mod.compile(waves_per_chain=W)
    expand_src = c._source.split("nphip_expand")[1]
    assert "nphip_kalman::smooth<1, 55, 2, true>(" in expand_src and "nphip_kalman::forward<1, 55, 2, true>(" in expand_src
    chains, draws, ahead = 8, 8, SMOOTHED_EXAMPLE["forecast"]
    tr = nutpie_amd.sample(c, chains=chains, tune=60, draws=draws, seed=3, progress_bar=False, store_unconstrained=True)
    n = chains * draws
    u = np.concatenate([np.asarray(tr.unconstrained_posterior[k].values).reshape(n, -1) for k in SCALES], axis=1)
    assert u.shape == (n, c.n_dim)
    host = c._expand_func(u, **c._data)
    if u.tobytes() not in references:      # (computed once where both W draw the same positions)
        references[u.tobytes()] = reported_references(mod, u)
    level, sd, pred_sd, e_level, e_sd = references[u.tobytes()]
    for name, e, want in (("smoothed_level", e_level, level), ("smoothed_level_sd", e_sd, sd)):
        got = tr.posterior[name].values.reshape(n, -1)
        on_host = np.asarray(host[name]).reshape(n, -1)
        assert got.shape == (n, 55)
        bound = 4.0 * e * np.abs(want).max()
        print(f"W = {W} {name}: device - host {np.abs(got - on_host).max():.3g}, device - 50 digits {np.abs(got - want).max():.3g}, "
              f"host - 50 digits {np.abs(on_host - want).max():.3g}, bound {bound:.3g} (53-bit recursion {e:.3g} of {np.abs(want).max():.3g})")
        assert e > 0.0
        assert np.abs(got - on_host).max() <= bound, name
        assert np.abs(got - want).max() <= bound, name
    got_sd = tr.posterior["smoothed_level_sd"].values.reshape(n, -1)
    bound = 4.0 * e_sd * np.abs(sd).max()
    print(f"W = {W} forecast sd: device - predicted {np.abs(got_sd[:, -ahead:] - pred_sd[:, -ahead:]).max():.3g}, bound {bound:.3g}")
    assert np.abs(got_sd[:, -ahead:] - pred_sd[:, -ahead:]).max() <= bound
    assert (np.diff(got_sd[:, -ahead:], axis=1) > 0.0).all()      # a forecast is less certain the further ahead


def test_smoothed_state_has_the_law_of_the_sampled_path(hip):
    """The two forms of the local level model of tests/test_gpu_kalman.py's law test, with its priors, target acceptance and run
    sizes (128 chains, tune 300, draws 200).  For every step t the mean over the draws of ``smoothed_state`` (marginal form) against
    the posterior mean of the sampled level x_t = l0 + sigma_level cumsum(z) (latent-path form), standard errors from each run's bulk
    ESS (nutpie_amd.ess): every |z| < 5.  Power: the mean of ``kalman_filtered_state`` breaks that condition at some step before
    the last — at the last step the two are the same quantity —, so the data do tell smoothing from filtering.
    Measured: the largest |z| of the smoothed mean 1.79; the filtered mean is off by up to 241 and breaks the condition at 36 steps."""
    from nutpie_amd.ess import ess_bulk

    T = LAW["T"]
    kw = dict(chains=128, tune=300, draws=200, target_accept=0.95, progress_bar=False)
    a = nutpie_amd.sample(local_level_smoothed().compile(), seed=11, **kw)
    b = nutpie_amd.sample(kalman_models.local_level_latent(**LAW).compile(), seed=12, **kw)
    shape = (kw["chains"], kw["draws"])
    smoothed = np.asarray(a.posterior["smoothed_state"].values).reshape(*shape, T)
    filtered = np.asarray(a.posterior["filtered_state"].values).reshape(*shape, T)
    l0 = np.asarray(b.posterior["l0"].values).reshape(*shape, 1)
    s_level = np.asarray(b.posterior["sigma_level"].values).reshape(*shape, 1)
    z = np.asarray(b.posterior["z"].values).reshape(*shape, T).copy()
    z[..., 0] = 0.0
    path = l0 + s_level * np.cumsum(z, axis=-1)

    def z_scores(mine):
        out = np.empty(T)
        for t in range(T):
            se = np.sqrt(mine[..., t].var() / ess_bulk(mine[..., t]) + path[..., t].var() / ess_bulk(path[..., t]))
            out[t] = (mine[..., t].mean() - path[..., t].mean()) / se
        return out

    z_s, z_f = z_scores(smoothed), z_scores(filtered)
    print("smoothed - path, |z| per step:", np.round(np.abs(z_s), 2).tolist())
    print("filtered - path, |z| per step:", np.round(np.abs(z_f), 2).tolist())
    assert np.isfinite(z_s).all() and (np.abs(z_s) < 5.0).all(), np.abs(z_s).max()
    assert (np.abs(z_f[:-1]) >= 5.0).any(), np.abs(z_f[:-1]).max()
